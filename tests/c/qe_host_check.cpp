// Host check of the quadratic-exponential step the device kernel shares with the host (csrc/hh_qe.h): reads lines of
//   kappa theta sigma rho r dt psi_c v x zv zx U martingale        (hex floats; martingale 0 / 1)
// from the file named on the command line, takes one step of each with hh_qe.h's functions exactly as hh_qe.hip's
// qe_member_step does, and prints "branch v' x'" (branch: 0 quadratic, 1 exponential with v' > 0, 2 its U <= p arm; hex
// floats).  tests/test_qe_host.py holds the printed values to the Python-float restatement, bit for bit, and builds
// the program twice — plainly, and with -fsanitize=address,undefined.
// The program itself evaluates every step again in long double from the raw parameters and fails (exit 3) when the
// fp64 step is further from it than kTol·scale: the step is about twenty rounded operations whose errors are amplified
// by at most ~10 (t = 2/ψ into b² into a), so 450 ε = 1e-13 of the larger of the value and its operands' scale (m for
// v', 1 for the log-spot increment) is generous for rounding and tiny against any wrong formula.  A state whose ψ lies
// within 1e-9 of ψ_c is printed but not compared: there the two precisions may take different branches.
#include <cmath>
#include <cstdio>

#include "../../hedgehog.jl_amd/csrc/hh_qe.h"

namespace {

constexpr long double kTol = 1e-13L;

struct Row {
  double kappa, theta, sigma, rho, r, dt, psi_c, v, x, zv, zx, U;
  int mart;
};

// the step in long double, straight from the header's formulas
void step_long(const Row& w, long double& vn, long double& xn, long double& m, long double& psi) {
  const long double k = w.kappa, th = w.theta, s = w.sigma, rho = w.rho, dt = w.dt, v = w.v;
  const long double E = expl(-k * dt), ome = 1.0L - E;
  m = th * ome + v * E;
  const long double s2 = v * (s * s * E * ome / k) + th * s * s * ome * ome / (2.0L * k);
  psi = s2 / (m * m);
  const long double psi_c = w.psi_c == 0.0 ? 1.5L : (long double)w.psi_c;
  const long double h = 0.5L * dt * (k * rho / s - 0.5L);
  const long double K0 = -rho * k * th * dt / s, K1 = h - rho / s, K2 = h + rho / s, K3 = 0.5L * dt * (1.0L - rho * rho);
  const long double A = K2 + 0.5L * K3;
  long double lnM;
  if (psi <= psi_c) {
    const long double t = 2.0L / psi, b2 = t - 1.0L + sqrtl(t) * sqrtl(t - 1.0L), a = m / (1.0L + b2);
    const long double bz = sqrtl(b2) + (long double)w.zv;
    vn = a * bz * bz;
    lnM = A * b2 * a / (1.0L - 2.0L * A * a) - 0.5L * logl(1.0L - 2.0L * A * a);
  } else {
    const long double p = (psi - 1.0L) / (psi + 1.0L), beta = (1.0L - p) / m;
    vn = (long double)w.U <= p ? 0.0L : logl((1.0L - p) / (1.0L - (long double)w.U)) / beta;
    lnM = logl(p + beta * (1.0L - p) / (beta - A));
  }
  const long double k0 = w.mart ? -lnM - (K1 + 0.5L * K3) * v : K0;
  xn = (long double)w.x + (long double)w.r * dt + k0 + K1 * v + K2 * vn + sqrtl(K3 * v + K3 * vn) * (long double)w.zx;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s rows.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  static_assert(sizeof(hh_qe) == 16, "hh_qe is a double and two int32");
  static_assert(sizeof(hh::QeArgs) == 13 * sizeof(double), "QeArgs is thirteen doubles");
  Row w;
  int bad = 0, compared[2] = {0, 0};
  while (std::fscanf(f, "%la %la %la %la %la %la %la %la %la %la %la %la %d", &w.kappa, &w.theta, &w.sigma, &w.rho, &w.r,
                     &w.dt, &w.psi_c, &w.v, &w.x, &w.zv, &w.zx, &w.U, &w.mart) == 13) {
    const hh::QeArgs q = hh::qe_args(w.kappa, w.theta, w.sigma, w.rho, w.r, w.dt, w.psi_c);
    const hh::QeMoments mo = hh::qe_moments(q, w.v);
    double vn, k0 = q.K0;
    int branch;
    if (mo.psi <= q.psi_c) {
      const hh::QeQuad b = hh::qe_quad(mo);
      vn = hh::qe_quad_next(b, w.zv);
      if (w.mart) k0 = hh::qe_k0_star(q, hh::qe_quad_lnM(b, q.A), w.v);
      branch = 0;
    } else {
      const hh::QeExp e = hh::qe_exp(mo);
      vn = hh::qe_exp_next(e, w.U);
      if (w.mart) k0 = hh::qe_k0_star(q, hh::qe_exp_lnM(e, q.A), w.v);
      branch = w.U <= e.p ? 2 : 1;
    }
    const double xn = hh::qe_log_spot(q, w.x, w.v, vn, k0, w.zx);
    std::printf("%d %a %a\n", branch, vn, xn);
    if (!(vn >= 0.0) || !std::isfinite(xn)) ++bad;
    long double vl, xl, ml, psil;
    step_long(w, vl, xl, ml, psil);
    if (fabsl(psil - (long double)q.psi_c) <= 1e-9L) continue;
    ++compared[branch != 0];
    const long double ev = fabsl((long double)vn - vl), exx = fabsl((long double)xn - xl);
    const long double sv = fmaxl(fabsl(vl), ml), sx = fmaxl(fabsl(xl - (long double)w.x), 1.0L);
    if (ev > kTol * sv || exx > kTol * sx) {
      std::fprintf(stderr, "row: v %a dt %a branch %d: v' off by %Lg (scale %Lg), x' by %Lg\n", w.v, w.dt, branch, ev, sv, exx);
      ++bad;
    }
  }
  std::fclose(f);
  std::fprintf(stderr, "compared %d quadratic, %d exponential steps; %d bad\n", compared[0], compared[1], bad);
  if (compared[0] == 0 || compared[1] == 0) return 4;
  return bad ? 3 : 0;
}
