// A host program on csrc/hh_localvol.h — the row and weight of a step, the bilinear lookup and the log-Euler step the
// device kernel (hh_localvol.hip) runs, compiled by a host compiler with -ffp-contract=off, plainly and under the host
// sanitizers (tests/test_localvol_host.py builds and runs it; nothing is loaded into an interpreter).
//
//   localvol_host_check <file>
// The file's lines, every number a hex float:
//   T n_times n_x x_lo h  times[n_times]  vols[n_times·n_x]     a surface, for the Q lines that follow
//   Q t x r dt dW                                               one lookup-and-step
// stdout, per Q line:  j  w  where  sigma  x′   (where: -1 clamped below, +1 above, 0 inside the grid)
// stderr: how many steps were compared with a long-double evaluation of the same formulas and how many lie further than
// 1e-13 from it; the exit status is 1 when any does.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hedgehog.jl_amd/csrc/hh_localvol.h"

namespace {

double hexf(const std::string& s) { return std::strtod(s.c_str(), nullptr); }

struct Surface {
  uint32_t n_times = 0, n_x = 0;
  double x_lo = 0.0, h = 1.0;
  std::vector<double> times, vols;
};

// the same lookup and step in long double, with the division by h the definition writes
void long_double_step(const Surface& s, double t, double x, double r, double dt, double dW, long double* sigma,
                      long double* xn) {
  uint32_t j = 0;
  long double w = 0.0L;
  if (s.n_times > 1u) {
    while (j + 2u < s.n_times && s.times[j + 1u] <= t) ++j;
    w = ((long double)t - s.times[j]) / ((long double)s.times[j + 1u] - s.times[j]);
    w = w < 0.0L ? 0.0L : w > 1.0L ? 1.0L : w;
  }
  long double u = ((long double)x - s.x_lo) / (long double)s.h;
  const long double top = (long double)(s.n_x - 1u);
  u = u < 0.0L ? 0.0L : u > top ? top : u;
  uint32_t i = (uint32_t)u;
  i = i < s.n_x - 2u ? i : s.n_x - 2u;
  const long double f = u - (long double)i;
  const double* a = s.vols.data() + (size_t)j * s.n_x;
  long double c0 = a[i], c1 = a[i + 1u];
  if (s.n_times > 1u) {
    const double* b = a + s.n_x;
    c0 = c0 + w * ((long double)b[i] - c0);
    c1 = c1 + w * ((long double)b[i + 1u] - c1);
  }
  const long double sg = c0 + f * (c1 - c0);
  *sigma = sg;
  *xn = (long double)x + (long double)dt * ((long double)r - 0.5L * sg * sg) + sg * (long double)dW;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <file>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  Surface s;
  std::string line;
  unsigned long compared = 0, bad = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string kind;
    ls >> kind;
    std::vector<std::string> tok;
    for (std::string t; ls >> t;) tok.push_back(t);
    if (kind == "T") {
      if (tok.size() < 4) return 2;
      s.n_times = (uint32_t)std::strtoul(tok[0].c_str(), nullptr, 10);
      s.n_x = (uint32_t)std::strtoul(tok[1].c_str(), nullptr, 10);
      const size_t n_nodes = (size_t)s.n_times * s.n_x;
      if (s.n_times < 1u || s.n_x < 2u || n_nodes > (size_t)HH_LV_MAX_NODES || tok.size() != 4 + s.n_times + n_nodes) return 2;
      s.x_lo = hexf(tok[2]);
      s.h = hexf(tok[3]);
      s.times.assign(s.n_times, 0.0);
      s.vols.assign(n_nodes, 0.0);
      for (uint32_t j = 0; j < s.n_times; ++j) s.times[j] = hexf(tok[4 + j]);
      for (size_t q = 0; q < n_nodes; ++q) s.vols[q] = hexf(tok[4 + s.n_times + q]);
    } else if (kind == "Q") {
      if (tok.size() != 5 || s.n_times == 0u) return 2;
      const double t = hexf(tok[0]), x = hexf(tok[1]), r = hexf(tok[2]), dt = hexf(tok[3]), dW = hexf(tok[4]);
      const hh::LocalVolRow row = hh::localvol_row(s.times.data(), s.n_times, t);
      const double inv_h = 1.0 / s.h;
      const hh::LocalVolCell c = hh::localvol_cell(x, s.x_lo, inv_h, s.n_x);
      const double u = (x - s.x_lo) * inv_h;
      const int where = u < 0.0 ? -1 : u > (double)(s.n_x - 1u) ? 1 : 0;
      const bool two = s.n_times > 1u;
      const double* a = s.vols.data() + (size_t)row.j * s.n_x;
      const double* b = a + (two ? s.n_x : 0u);
      const double sigma = hh::localvol_sigma(a, b, two, c, row.w);
      const double xn = hh::localvol_step(x, sigma, r, dt, dW);
      std::printf("%u %a %d %a %a\n", row.j, row.w, where, sigma, xn);
      long double sl, xl;
      long_double_step(s, t, x, r, dt, dW, &sl, &xl);
      ++compared;
      if (!(fabsl((long double)sigma - sl) <= 1e-13L) || !(fabsl((long double)xn - xl) <= 1e-13L)) {
        ++bad;
        std::fprintf(stderr, "t=%a x=%a: sigma %a (long double %La), x' %a (long double %La)\n", t, x, sigma, sl, xn, xl);
      }
    } else if (!kind.empty()) {
      return 2;
    }
  }
  std::fprintf(stderr, "compared %lu steps; %lu bad\n", compared, bad);
  return bad ? 1 : 0;
}
