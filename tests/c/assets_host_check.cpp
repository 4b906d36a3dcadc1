// Host check of what a multi-asset call forms on the host (csrc/hh_assets.h): the checks of the correlation matrix,
// its Cholesky factor and the step's constants.  Reads records from the file named on the command line —
//   d kind n_steps r T, then d spots, d sigmas, d weights and the d·d correlations row by row, numbers as hex floats
// — and prints for each either "invalid <reason>" or "ok" followed by L (packed), drift, A (packed) and x0 in hex.
// tests/test_assets_host.py builds it twice — plainly, and with -fsanitize=address,undefined — and holds every number
// to the Python-float restatement bit for bit.  Built with -ffp-contract=off, as the library is.
#include <cmath>
#include <cstdio>

#include "../../hedgehog.jl_amd/csrc/hh_assets.h"

static void put(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s records.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  static_assert(sizeof(hh_assets) == 8 + 3 * 64 + 512, "hh_assets: two words, three vectors, one matrix");
  static_assert(sizeof(hh::AssetArgs) == (8 + 8 + 8 + 36) * sizeof(double), "AssetArgs: 60 doubles by value");
  unsigned d, n_steps, seen = 0, bad = 0;
  int kind;
  double r, T;
  while (std::fscanf(f, "%u %d %u %la %la", &d, &kind, &n_steps, &r, &T) == 5) {
    if (d < 1 || d > HH_MAX_ASSETS) return 3;
    hh_assets as{};
    as.n_assets = d;
    as.index_kind = kind;
    bool read = true;
    for (unsigned i = 0; i < d; ++i) read = read && std::fscanf(f, "%la", &as.spots[i]) == 1;
    for (unsigned i = 0; i < d; ++i) read = read && std::fscanf(f, "%la", &as.sigmas[i]) == 1;
    for (unsigned i = 0; i < d; ++i) read = read && std::fscanf(f, "%la", &as.weights[i]) == 1;
    for (unsigned i = 0; i < d; ++i)
      for (unsigned j = 0; j < d; ++j) read = read && std::fscanf(f, "%la", &as.corr[i * HH_MAX_ASSETS + j]) == 1;
    if (!read) return 3;
    ++seen;
    double L[hh::kAssetsTri] = {};
    if (const char* defect = hh::corr_defect(as)) {
      std::printf("invalid %s\n", defect);
      ++bad;
      continue;
    }
    if (!hh::cholesky(as.corr, d, L)) {
      std::printf("invalid not positive definite\n");
      ++bad;
      continue;
    }
    const hh::AssetArgs a = hh::asset_args(as, r, T, n_steps, L);
    const int tri = (int)(d * (d + 1) / 2);
    std::printf("ok");
    put(L, tri);
    put(a.drift, (int)d);
    put(a.A, tri);
    put(a.x0, (int)d);
    std::printf("\n");
  }
  std::fclose(f);
  std::fprintf(stderr, "read %u records; %u invalid\n", seen, bad);
  return 0;
}
