// Host check of the Crank–Nicolson scheme the device kernels share with the host (csrc/hh_fd.h): reads one option per
// line — "S0 K cp sigma r T W style M N R", the doubles as hex floats — from the file named on the command line, prices
// each with the header's serial step and prints price, delta and gamma as hex floats.  It also holds the header's map
// composition to applying the maps one after the other.  tests/test_fd_host.py builds it twice — plainly, and with
// -fsanitize=address,undefined — and holds the output to the bars of the 50-digit restatement.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../hedgehog.jl_amd/csrc/hh_fd.h"

static int price(double S0, double K, double cp, double sigma, double r, double T, double W, int style, int M, int N, int R,
                 double out[3]) {
  if (M < 4 || M > HH_FD_MAX_SPACE || (M & 1) || N < 1 || N > HH_FD_MAX_TIME || R < 0 || R > N) return 1;
  const int half = M / 2;
  const double h = W / (double)half;
  const hh::FdCoef c = hh::fd_coef(sigma, r, h);
  if (!hh::fd_coef_ok(c)) return 1;
  const bool american = style == HH_FD_AMERICAN;
  const double x0 = std::log(S0);
  std::vector<double> S(M + 1), g(M + 1), V(M + 1), piv(M + 1), y(M + 1);
  for (int j = 0; j <= M; ++j) {
    S[j] = std::exp(x0 + (double)(j - half) * h);
    g[j] = hh::fd_max(cp * (S[j] - K), 0.0);
    V[j] = g[j];
  }
  const double dt = T / (double)N;
  double tau = 0.0;
  for (int n = 0; n < N; ++n) {
    const bool rann = n < R;
    const double k = rann ? 0.5 * dt : dt;
    const hh::FdPhase p = hh::fd_phase(c, k, rann ? 1.0 : 0.5);
    for (int s = 0; s < (rann ? 2 : 1); ++s) {
      tau = tau + k;
      const double disc = std::exp(-r * tau);
      const double v0 = cp > 0.0 ? 0.0 : (american ? K - S[0] : K * disc - S[0]);
      const double vM = cp > 0.0 ? S[M] - K * disc : 0.0;
      hh::fd_serial_step(V.data(), g.data(), piv.data(), y.data(), M, c, p, cp, american, v0, vM);
    }
  }
  const double d1 = (V[half + 1] - V[half - 1]) / (2.0 * h);
  const double d2 = ((V[half + 1] - 2.0 * V[half]) + V[half - 1]) / (h * h);
  out[0] = V[half];
  out[1] = d1 / S0;
  out[2] = (d2 - d1) / (S0 * S0);
  return 0;
}

// composing then applying equals applying in turn, up to the roundings of the two orders
static int check_maps() {
  const hh::FdMap f1{0.5, 1.25, 0.75}, f2{0.25, -0.5, 0.125}, f3{0.75, 2.0, -1.0e300};
  const hh::FdMap f = hh::fd_compose(f3, hh::fd_compose(f2, f1));
  for (double x = -4.0; x <= 4.0; x += 0.125) {
    const double a = hh::fd_apply(f, x), b = hh::fd_apply(f3, hh::fd_apply(f2, hh::fd_apply(f1, x)));
    if (std::fabs(a - b) > 1e-15 * (1.0 + std::fabs(b))) return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s options.txt\n", argv[0]);
    return 2;
  }
  if (check_maps()) return 4;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  double d[7];
  int style, M, N, R;
  while (std::fscanf(f, "%la %la %la %la %la %la %la %d %d %d %d", &d[0], &d[1], &d[2], &d[3], &d[4], &d[5], &d[6], &style,
                     &M, &N, &R) == 11) {
    double out[3];
    if (price(d[0], d[1], d[2], d[3], d[4], d[5], d[6], style, M, N, R, out)) {
      std::fclose(f);
      return 3;
    }
    std::printf("%a %a %a\n", out[0], out[1], out[2]);
  }
  std::fclose(f);
  return 0;
}
