// Host program around csrc/hh_vg.h's gamma_mt (tests/test_vg_host.py builds it plainly and with
// -fsanitize=address,undefined and runs it as a program; nothing of it is loaded into an interpreter).
//
//   vg_host_check fixture <file>
//       every line of the file: span nu n  z_0 U_0 U'_0 … z_{n−1} U_{n−1} U'_{n−1}   (hex doubles; σ = r = θ = 0)
//       prints per line: the attempts made, the variate (hex) — and fails when the sampler asks for an attempt the line
//       does not hold.
//   vg_host_check law <span> <nu> <n> <seed>
//       n variates of Gamma(span/nu, nu) on Philox draws of this program's own: trajectory i of key `seed`, attempt t:
//       z the first Box–Muller normal of block (i, t, 0, 8), U and U′ from block (i, t, 1, 8).  Prints them (hex).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hedgehog.jl_amd/csrc/hh_vg.h"

namespace {

struct ListedDraws {
  std::vector<hh::VgDraws> draws;
  bool ran_out = false;
  hh::VgDraws attempt(uint32_t t) {
    if (t >= draws.size()) {
      ran_out = true;
      return hh::VgDraws{0.0, 0.5, 0.5};
    }
    return draws[t];
  }
};

// Philox4x32-10 (Salmon et al., SC'11) and the library's uniform, restated for the host
void philox(const uint32_t ctr[4], uint64_t key, uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
double u01(uint32_t lo, uint32_t hi) {
  const uint64_t w = ((uint64_t)hi << 32) | lo;
  return ((double)(w >> 12) + 0.5) * 0x1p-52;
}

struct PhiloxDraws {
  uint32_t path;
  uint64_t key;
  hh::VgDraws attempt(uint32_t t) const {
    uint32_t a[4], b[4];
    const uint32_t ca[4] = {path, t, 0u, 8u}, cb[4] = {path, t, 1u, 8u};
    philox(ca, key, a);
    philox(cb, key, b);
    const double r = std::sqrt(-2.0 * std::log(u01(a[0], a[1])));
    return hh::VgDraws{r * std::cos(6.283185307179586476925 * u01(a[2], a[3])), u01(b[0], b[1]), u01(b[2], b[3])};
  }
};

hh_vg vg_of(double nu) {
  hh_vg g;
  g.theta = 0.0;
  g.nu = nu;
  return g;
}

int run_fixture(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string tok;
    std::vector<double> v;
    while (ss >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
    if (v.size() < 3 || v.size() != 3 + 3 * (size_t)v[2]) return 3;
    const hh::VgArgs g = hh::vg_args(0.0, 0.0, vg_of(v[1]), v[0]);
    ListedDraws src;
    for (size_t t = 0; t < (size_t)v[2]; ++t) src.draws.push_back(hh::VgDraws{v[3 + 3 * t], v[4 + 3 * t], v[5 + 3 * t]});
    uint32_t attempts = 0;
    const double G = hh::gamma_mt(g, src, &attempts);
    if (src.ran_out) {
      std::fprintf(stderr, "the sampler asked for more attempts than the line holds: %s\n", line.c_str());
      return 4;
    }
    std::printf("%" PRIu32 " %a\n", attempts, G);
  }
  return 0;
}

int run_law(double span, double nu, long n, uint64_t seed) {
  const hh::VgArgs g = hh::vg_args(0.0, 0.0, vg_of(nu), span);
  for (long i = 0; i < n; ++i) {
    PhiloxDraws src{(uint32_t)i, seed};
    std::printf("%a\n", hh::gamma_mt(g, src));
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "fixture")) return run_fixture(argv[2]);
  if (argc == 6 && !std::strcmp(argv[1], "law"))
    return run_law(std::strtod(argv[2], nullptr), std::strtod(argv[3], nullptr), std::strtol(argv[4], nullptr, 10),
                   std::strtoull(argv[5], nullptr, 0));
  std::fprintf(stderr, "usage: vg_host_check fixture <file> | law <span> <nu> <n> <seed>\n");
  return 1;
}
