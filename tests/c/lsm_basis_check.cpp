// The regression basis of the several-variable induction on the host (csrc/hh_lsm_basis.h), as a program of its own: for
// every (m, p), m = 1 .. 9, p = 0 .. 9, one line
//   m p B word_0 … word_{B−1} | phi_0 … phi_{B−1}
// — the count (0: not admitted), the exponent words in the header's order and lsm_phi of each on the fixed regressors
// z_i = (i + 2)/8 − 1 (hex floats) — then a line with the padding's φ.  tests/test_assets_lsm_host.py holds the lines to the
// Python restatement; built with -fsanitize=address,undefined it also shows the enumeration writes inside its table.
#include <cstdio>

#include "../../hedgehog.jl_amd/csrc/hh_lsm_basis.h"

template <int M>
static void phis(const uint32_t* words, int B) {
  double z[M];
  for (int i = 0; i < M; ++i) z[i] = (i + 2) / 8.0 - 1.0;
  for (int j = 0; j < B; ++j) std::printf(" %a", hh::lsm_phi<M, hh::lsm_max_degree(M)>(1.0, z, words[j]));
}

int main() {
  for (int m = 1; m <= 9; ++m)
    for (int p = 0; p <= 9; ++p) {
      uint32_t words[hh::kLsmBasisPad];
      const int B = hh::lsm_basis_fill(m, p, words);
      if (B != hh::lsm_basis_count(m, p)) return 1;
      for (int j = B; j < hh::kLsmBasisPad; ++j)
        if (words[j] != hh::kLsmNoBasis) return 2;
      std::printf("%d %d %d", m, p, B);
      for (int j = 0; j < B; ++j) std::printf(" %x", words[j]);
      std::printf(" |");
      switch (m) {
        case 1: phis<1>(words, B); break;
        case 2: phis<2>(words, B); break;
        case 3: phis<3>(words, B); break;
        case 4: phis<4>(words, B); break;
        case 5: phis<5>(words, B); break;
        case 6: phis<6>(words, B); break;
        case 7: phis<7>(words, B); break;
        case 8: phis<8>(words, B); break;
        default: break;
      }
      std::printf("\n");
    }
  const double z[2] = {0.5, -3.0};
  std::printf("padding %a %a\n", hh::lsm_phi<2, 7>(1.0, z, hh::kLsmNoBasis), hh::lsm_phi<2, 7>(0.0, z, 0x21u));
  for (int m = 1; m <= 8; ++m) std::printf("max_degree %d %d\n", m, hh::lsm_max_degree(m));
  return 0;
}
