// Host check of the Poisson inversion the Merton kernels share with the host (csrc/hh_jump.h): reads "U m" pairs (hex
// floats, one pair per line) from the file named on the command line and prints the jump count of each, forming
// p0 = exp(-m) as the library's host code does.  tests/test_merton_host.py builds it twice — plainly, and with
// -fsanitize=address,undefined — and holds the counts to the 50-digit restatement.  A search that did not end would
// hang this program: the cap HH_JUMP_MAX_COUNT is what ends it where the fp64 cumulative sum saturates.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../hedgehog.jl_amd/csrc/hh_jump.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s pairs.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<double> u, m;
  double a, b;
  while (std::fscanf(f, "%la %la", &a, &b) == 2) {
    u.push_back(a);
    m.push_back(b);
  }
  std::fclose(f);
  for (size_t i = 0; i < u.size(); ++i) {
    const uint32_t n = hh::poisson_inverse(u[i], m[i], std::exp(-m[i]));
    if (n > (uint32_t)HH_JUMP_MAX_COUNT) return 3;
    std::printf("%u\n", n);
  }
  static_assert(sizeof(hh_jump) == 24, "hh_jump is three doubles");
  static_assert(sizeof(hh::JumpArgs) == 32, "JumpArgs is four doubles");
  return 0;
}
