// What a multi-asset call forms ONCE on the host (include/hedgehog_mc.h, "Several correlated lognormal assets" — every
// operation is stated there in this order): the checks of the correlation matrix, its Cholesky factor, and the step's
// constants packed into the by-value argument block of the kernels (hh_assets.hip).  It includes nothing of HIP, so
// that tests/c/assets_host_check.cpp can hold it to a Python-float restatement bit for bit and run it under the host
// sanitizers.  Every operation is one rounded fp64 operation (the library is built with -ffp-contract=off; a host
// program that includes this must be too).  Internal; the public surface is include/hedgehog_mc.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

namespace hh {

constexpr int kAssetsTri = HH_MAX_ASSETS * (HH_MAX_ASSETS + 1) / 2;  // entries of a packed lower triangle

// entry (i, j), j <= i, of a packed lower triangle: rows one after the other
inline constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// The constants of a launch, passed BY VALUE (wave-uniform).  Entries at or beyond n_assets are zero and never read.
struct AssetArgs {
  double drift[HH_MAX_ASSETS];  // (r − σ_i²/2)·dt
  double x0[HH_MAX_ASSETS];     // log spot_i; best-of / worst-of: + log w_i
  double w[HH_MAX_ASSETS];      // the weights of a weighted sum or a geometric mean
  double A[kAssetsTri];         // (σ_i·L_ij)·sqrt(dt), packed by tri(i, j)
};

// What is wrong with the correlation matrix before any factorisation, or nullptr.
inline const char* corr_defect(const hh_assets& as) {
  const uint32_t d = as.n_assets;
  for (uint32_t i = 0; i < d; ++i)
    for (uint32_t j = 0; j < d; ++j) {
      const double c = as.corr[i * HH_MAX_ASSETS + j];
      if (!isfinite(c) || !(fabs(c) <= 1.0)) return "a correlation is not finite or lies outside [-1, 1]";
    }
  for (uint32_t i = 0; i < d; ++i)
    if (as.corr[i * HH_MAX_ASSETS + i] != 1.0) return "the correlation matrix's diagonal must be 1";
  for (uint32_t i = 0; i < d; ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (as.corr[i * HH_MAX_ASSETS + j] != as.corr[j * HH_MAX_ASSETS + i]) return "the correlation matrix is not symmetric";
  return nullptr;
}

// Cholesky–Banachiewicz, row by row, of the d × d matrix C (row stride HH_MAX_ASSETS) into the packed triangle L:
//   s = C_ij;  s = s − L_ik·L_jk for k = 0 … j−1 in this order (a rounded product, then a rounded subtraction);
//   L_ij = s / L_jj (j < i),  L_ii = sqrt(s).
// false: a diagonal s is not > 0 or not finite — the matrix is not positive definite; L is then unspecified.
inline bool cholesky(const double* C, uint32_t d, double* L) {
  for (uint32_t i = 0; i < d; ++i)
    for (uint32_t j = 0; j <= i; ++j) {
      double s = C[i * HH_MAX_ASSETS + j];
      for (uint32_t k = 0; k < j; ++k) s = s - L[tri(i, k)] * L[tri(j, k)];
      if (j < i) {
        L[tri(i, j)] = s / L[tri(j, j)];
      } else {
        if (!(s > 0.0) || !isfinite(s)) return false;
        L[tri(i, i)] = sqrt(s);
      }
    }
  return true;
}

// The step's constants, in the header's order; L from cholesky().  The assets have passed the entry point's checks.
inline AssetArgs asset_args(const hh_assets& as, double r_drift, double T, uint32_t n_steps, const double* L) {
  AssetArgs a{};
  const double dt = T / (double)n_steps;
  const double sqrt_dt = sqrt(dt);
  const bool extreme = as.index_kind == HH_INDEX_BEST_OF || as.index_kind == HH_INDEX_WORST_OF;
  for (uint32_t i = 0; i < as.n_assets; ++i) {
    const double sig = as.sigmas[i];
    const double sig2h = 0.5 * sig * sig;  // as make_args forms it
    a.drift[i] = (r_drift - sig2h) * dt;
    for (uint32_t j = 0; j <= i; ++j) a.A[tri(i, j)] = (sig * L[tri(i, j)]) * sqrt_dt;
    a.x0[i] = extreme ? log(as.spots[i]) + log(as.weights[i]) : log(as.spots[i]);
    a.w[i] = as.weights[i];
  }
  return a;
}

// ---- what the kernels share (hh_assets.hip: the statistics and the state rows; hh_lsm_multi.hip: the exercise value on a
// stored row) — device code, seen by hipcc alone ----
#if defined(__HIPCC__)
}  // namespace hh
#include "hh_path_stats.h"  // vmax, vmin
namespace hh {
namespace {

// the pair (I, x) of the index on a date — what Running::first / next take as (S, log S)
template <int D, int KIND>
__device__ __forceinline__ void index_of(const AssetArgs& c, const double (&x)[D], double& I, double& xi) {
  if constexpr (KIND == HH_INDEX_WEIGHTED_SUM) {
    I = c.w[0] * exp(x[0]);
#pragma unroll
    for (int i = 1; i < D; ++i) I = fma(c.w[i], exp(x[i]), I);
    xi = log(I);
  } else if constexpr (KIND == HH_INDEX_GEOMETRIC) {
    xi = c.w[0] * x[0];
#pragma unroll
    for (int i = 1; i < D; ++i) xi = fma(c.w[i], x[i], xi);
    I = exp(xi);
  } else {  // best-of, worst-of: log w_i is in the initial state
    xi = x[0];
#pragma unroll
    for (int i = 1; i < D; ++i) xi = KIND == HH_INDEX_BEST_OF ? vmax(xi, x[i]) : vmin(xi, x[i]);
    I = exp(xi);
  }
}

// x_i += drift_i + Σ_{j<=i} A_ij·(±z_j), the sum as a chain of fma in j
template <int D, bool MIRROR>
__device__ __forceinline__ void step_assets(const AssetArgs& c, double (&x)[D], const double (&z)[2 * ((D + 1) / 2)]) {
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double acc = c.drift[i];
#pragma unroll
    for (int j = 0; j <= i; ++j) acc = fma(c.A[tri(i, j)], MIRROR ? -z[j] : z[j], acc);
    x[i] = x[i] + acc;
  }
}

}  // namespace
#endif  // __HIPCC__

}  // namespace hh
