// Host check of the Bates step the device kernel shares with the host (csrc/hh_qe.h, csrc/hh_jump.h): reads lines of
//   kappa theta sigma rho r dt psi_c lambda mu_j sigma_j v x zv zx U UJ z martingale mirror
// (hex floats; martingale, mirror 0 / 1) from the file named on the command line and takes one step of each exactly as
// hh_bates.hip's kernel does: the constants by qe_args on r_c = r − merton_compensator(jump), the member's draws
// (the mirror takes −zv, −zx, 1 − U and −z), the QE step, N = poisson_inverse(UJ, mean, p0) with jump_args' mean and
// p0, and x′ + jump_sum(N, ±z) where N > 0.  It prints "branch N v' x'" (branch: 0 quadratic, 1 exponential with v' > 0,
// 2 its U <= p arm; hex floats).  tests/test_bates_host.py holds the printed values to the Python-float restatement of
// tests/bates_cases.py, bit for bit, and builds the program twice — plainly, and with -fsanitize=address,undefined.
// The program fails (exit 3) on a step that is not finite or a count above HH_JUMP_MAX_COUNT, and (exit 4) when its rows
// did not reach both branches, both members and every N of 0 … 4.
#include <cmath>
#include <cstdio>

#include "../../hedgehog.jl_amd/csrc/hh_jump.h"
#include "../../hedgehog.jl_amd/csrc/hh_qe.h"

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
  static_assert(sizeof(hh_jump) == 24, "hh_jump is three doubles");
  static_assert(sizeof(hh::JumpArgs) == 4 * sizeof(double), "JumpArgs is four doubles");
  double kappa, theta, sigma, rho, r, dt, psi_c, v, x, zv, zx, U, UJ, z;
  hh_jump jump;
  int mart, mirror, bad = 0, rows = 0, seen_branch[3] = {0, 0, 0}, seen_N[5] = {0, 0, 0, 0, 0}, seen_member[2] = {0, 0};
  while (std::fscanf(f, "%la %la %la %la %la %la %la %la %la %la %la %la %la %la %la %la %la %d %d", &kappa, &theta, &sigma,
                     &rho, &r, &dt, &psi_c, &jump.lambda, &jump.mu_j, &jump.sigma_j, &v, &x, &zv, &zx, &U, &UJ, &z, &mart,
                     &mirror) == 19) {
    const double r_c = r - hh::merton_compensator(jump);
    const hh::QeArgs q = hh::qe_args(kappa, theta, sigma, rho, r_c, dt, psi_c);
    const hh::JumpArgs j = hh::jump_args(jump, dt);
    if (mirror) {
      zv = -zv;
      zx = -zx;
      U = 1.0 - U;
      z = -z;
    }
    const hh::QeMoments mo = hh::qe_moments(q, v);
    double vn, k0 = q.K0;
    int branch;
    if (mo.psi <= q.psi_c) {
      const hh::QeQuad b = hh::qe_quad(mo);
      vn = hh::qe_quad_next(b, zv);
      if (mart) k0 = hh::qe_k0_star(q, hh::qe_quad_lnM(b, q.A), v);
      branch = 0;
    } else {
      const hh::QeExp e = hh::qe_exp(mo);
      vn = hh::qe_exp_next(e, U);
      if (mart) k0 = hh::qe_k0_star(q, hh::qe_exp_lnM(e, q.A), v);
      branch = U <= e.p ? 2 : 1;
    }
    double xn = hh::qe_log_spot(q, x, v, vn, k0, zx);
    const uint32_t N = hh::poisson_inverse(UJ, j.mean, j.p0);
    if (N > 0u) xn = xn + hh::jump_sum(j, N, z);
    std::printf("%d %u %a %a\n", branch, N, vn, xn);
    if (!(vn >= 0.0) || !std::isfinite(xn) || N > (uint32_t)HH_JUMP_MAX_COUNT) ++bad;
    ++rows;
    ++seen_branch[branch];
    ++seen_member[mirror != 0];
    if (N < 5u) ++seen_N[N];
  }
  std::fclose(f);
  std::fprintf(stderr, "stepped %d rows; %d bad\n", rows, bad);
  if (bad) return 3;
  for (int n : seen_branch)
    if (n == 0) return 4;
  for (int n : seen_N)
    if (n == 0) return 4;
  return seen_member[0] && seen_member[1] ? 0 : 4;
}
