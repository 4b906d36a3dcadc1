// The regression basis of the several-variable induction (hh_lsm_multi.hip; include/hedgehog_mc.h, "American exercise on
// several state rows"): all monomials Π z_i^{e_i}, i < m, of total degree <= p.
//
// ORDER — graded lexicographic, stated here once: by total degree 0, 1, …, p; within a degree the exponent tuples
// (e_0, …, e_{m−1}) in DESCENDING lexicographic order, e_0 compared first.  So m = 2, p = 2 is
//   1,  z_0, z_1,  z_0², z_0·z_1, z_1²
// and m = 1 is 1, z, z², …: the one-variable basis.  There are B = C(m + p, p) of them; HH_LSM_MAX_BASIS = 45 admits
// m = 8 and 7 at p <= 2, m = 6 and 5 at p <= 2, m = 4 at p <= 3, m = 3 at p <= 4, m = 2 and m = 1 at p <= 8 (C(10, 8) is 45 exactly).
//
// A monomial travels as one word, four bits per variable: e_i = (word >> 4·i) & 15.  Its VALUE is formed by lsm_phi and
// by nothing else: start, then times z_0 e_0 times, then times z_1 e_1 times, … — every product one rounded fp64
// operation, in this order.  The Gram sums, the moment sums and the fitted continuation value all call it, so they see
// the same φ bit for bit.
//
// Plain C++, nothing of HIP: tests/c/lsm_basis_check.cpp includes it and runs under the host sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

#if defined(__HIPCC__)
#define HH_BASIS_FN __host__ __device__ __forceinline__
#else
#define HH_BASIS_FN inline
#endif

namespace hh {

constexpr int kLsmMaxBasis = HH_LSM_MAX_BASIS;
constexpr int kLsmBasisPad = 48;  // entries of a padded table: three tiles of 16
constexpr uint32_t kLsmNoBasis = 0x80000000u;  // a padded table's entries at and beyond B: their φ is 0 whatever z

// C(m + p, p), or 0 where m, p are out of range or the count is above HH_LSM_MAX_BASIS
HH_BASIS_FN constexpr int lsm_basis_count(int m, int p) {
  if (m < 1 || m > HH_MAX_ASSETS || p < 1 || p > 8) return 0;
  int b = 1;
  for (int k = 1; k <= p; ++k) {  // C(m + k, k) = C(m + k − 1, k − 1)·(m + k)/k, exact at every k
    b = b * (m + k) / k;
    if (b > kLsmMaxBasis) return 0;
  }
  return b;
}

// the largest degree m variables admit
HH_BASIS_FN constexpr int lsm_max_degree(int m) {
  int p = 0;
  while (p < 8 && lsm_basis_count(m, p + 1) > 0) ++p;
  return p;
}

// The exponent words of the basis in the order above into out[kLsmBasisPad], padded with kLsmNoBasis; returns B, or 0
// where (m, p) is not admitted (out is then all padding).
inline int lsm_basis_fill(int m, int p, uint32_t* out) {
  for (int j = 0; j < kLsmBasisPad; ++j) out[j] = kLsmNoBasis;
  const int B = lsm_basis_count(m, p);
  if (B == 0) return 0;
  int n = 0;
  for (int deg = 0; deg <= p; ++deg) {
    int e[HH_MAX_ASSETS] = {};
    e[0] = deg;
    for (;;) {
      uint32_t w = 0;
      for (int i = 0; i < m; ++i) w |= (uint32_t)e[i] << (4 * i);
      out[n++] = w;
      // the next tuple of this degree in descending lexicographic order: take one from the last positive exponent in
      // front of the last place and hand it, with whatever the last place held, to the place behind it
      int i = m - 2;
      while (i >= 0 && e[i] == 0) --i;
      if (i < 0) break;
      const int last = e[m - 1];
      e[m - 1] = 0;
      --e[i];
      e[i + 1] = last + 1;
    }
  }
  return n;  // == B
}

// φ of the word e on the standardised regressors z: start·Π z_i^{e_i}, multiplied in the order of the head comment.
// P: the largest exponent M variables admit (lsm_max_degree(M)); p <= P: the degree of the caller's basis — no exponent of
// it is larger, so the steps k >= p are skipped (a uniform branch) without changing a bit.  The loops are unrolled in full
// and every product is a select, so z stays in registers.  start is 1 for a column that is in the money and 0 for one
// that is not.
template <int M, int P>
HH_BASIS_FN double lsm_phi(double start, const double (&z)[M], uint32_t e, int p = P) {
  double pw = (e & kLsmNoBasis) ? 0.0 : start;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < M; ++i) {
    const int ei = (int)((e >> (4 * i)) & 15u);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < P; ++k)
      if (k < p) pw = k < ei ? pw * z[i] : pw;
  }
  return pw;
}

}  // namespace hh
