// Bates (1996) for gfx950 (wave64, fp64 VALU): Heston variance by the quadratic-exponential step plus Merton jumps in
// log S (include/hedgehog_mc.h, "Bates (1996): Heston variance with Merton jumps" — the step, the draws and the
// host-formed constants are stated there in full).  The step's arithmetic is hh_qe.h's, the jump count and the jump sum
// are hh_jump.h's; both are shared with host programs.
//
//   bates_stats_kernel<ANTI, MART>  qe_stats_kernel's form — one trajectory per lane and its mirror in the same lane, the
//                                   same dates and Running arithmetic (hh_path_stats.h), the same five rows and var_T —
//                                   with jump_stats_kernel's two additions per step k: the jump count N_k from the
//                                   uniform of block (k >> 1, 0, 0, kDomJump) and, only where N_k > 0, the jump from the
//                                   first normal of block (k, 1, 0, kDomJump), added to x after the QE step and before
//                                   the date.  Its output goes through path_payoff_kernel untouched.
//
// QeArgs carries rdt = (r − λκ̄)·dt, the only place the compensator enters; JumpArgs travels beside it.  Every loop is
// bounded by n_steps or, the count search, by HH_JUMP_MAX_COUNT; none by data.  The block of jump uniforms is drawn on
// the even steps and its words 2, 3 are carried to the odd one: one block per two steps whatever n_steps is, an odd
// n_steps leaving the last block half read.  The exponential branch's block and the jump's block are drawn under a
// branch each.  With mean = 0 no lane ever jumps and every operation left on the states is qe_stats_kernel's.
#include "hh_jump.h"
#include "hh_path_stats.h"
#include "hh_qe.h"
#include "hh_sim.h"

namespace hh {
namespace {

struct BatesState {
  double x, v;
};

// (x, v) -> (x′, v′) of one member by the QE step: qe_stats_kernel's qe_member_step, operation for operation
template <bool MART>
__device__ __forceinline__ void bates_member_step(BatesState& s, const QeArgs& q, const QeMoments& mo, bool quad,
                                                  double zv, double zx, double U) {
  double vn, k0 = q.K0;
  if (quad) {
    const QeQuad b = qe_quad(mo);
    vn = qe_quad_next(b, zv);
    if constexpr (MART) k0 = qe_k0_star(q, qe_quad_lnM(b, q.A), s.v);
  } else {
    const QeExp e = qe_exp(mo);
    vn = qe_exp_next(e, U);
    if constexpr (MART) k0 = qe_k0_star(q, qe_exp_lnM(e, q.A), s.v);
  }
  s.x = qe_log_spot(q, s.x, s.v, vn, k0, zx);
  s.v = vn;
}

template <bool ANTI, bool MART>
__global__ __launch_bounds__(256) void bates_stats_kernel(const SimArgs<0> a, const QeArgs q, const JumpArgs j,
                                                          const double S0, const uint32_t monitor_every,
                                                          const int include_start, double* __restrict__ stats,
                                                          double* __restrict__ var_T) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  BatesState st{a.x0.v, a.v0.v}, sa{a.x0.v, a.v0.v};
  Running r, ra;
  bool started = include_start != 0;
  if (started) {
    r.first(S0, a.x0.v);
    if constexpr (ANTI) ra.first(S0, a.x0.v);
  }
  uint32_t left = monitor_every;
  const uint64_t key = a.seeds[i];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  uint32_t odd_lo = 0u, odd_hi = 0u;  // words 2, 3 of the even step's block of jump uniforms
  for (uint32_t k = 0; k < n_steps; ++k) {
    // the QE step on the draws of domain kDomQe
    double zv, zx;
    normal_pair(key, k, 0u, 0u, kDomQe, zv, zx);
    const QeMoments mo = qe_moments(q, st.v);
    const bool quad = mo.psi <= q.psi_c;
    QeMoments moa = mo;
    bool quada = true;
    if constexpr (ANTI) {
      moa = qe_moments(q, sa.v);
      quada = moa.psi <= q.psi_c;
    }
    double U = 0.5;  // read by a member in the exponential branch only
    if (!quad || !quada) {
      const Philox4 b = philox4x32_10(k, 1u, 0u, kDomQe, k0, k1);
      U = u01_fast(b.c0, b.c1);
    }
    bates_member_step<MART>(st, q, mo, quad, zv, zx, U);
    if constexpr (ANTI) bates_member_step<MART>(sa, q, moa, quada, -zv, -zx, 1.0 - U);  // 1 − U is exact
    // the jump on the draws of domain kDomJump: one block of uniforms per two steps
    double uj;
    if ((k & 1u) == 0u) {
      const Philox4 b = philox4x32_10(k >> 1, 0u, 0u, kDomJump, k0, k1);
      uj = u01_fast(b.c0, b.c1);
      odd_lo = b.c2;
      odd_hi = b.c3;
    } else {
      uj = u01_fast(odd_lo, odd_hi);
    }
    const uint32_t N = poisson_inverse(uj, j.mean, j.p0);
    if (N > 0u) {
      double z, unused;
      normal_pair(key, k, 1u, 0u, kDomJump, z, unused);
      st.x = st.x + jump_sum(j, N, z);
      if constexpr (ANTI) sa.x = sa.x + jump_sum(j, N, -z);
    }
    if (--left == 0u) {
      left = monitor_every;
      const double S = exp(st.x);
      if (started) r.next(S, st.x);
      else r.first(S, st.x);
      if constexpr (ANTI) {
        const double Sa = exp(sa.x);
        if (started) ra.next(Sa, sa.x);
        else ra.first(Sa, sa.x);
      }
      started = true;
    }
  }
  r.store(stats, at, i);
  if (var_T) var_T[i] = st.v;
  if constexpr (ANTI) {
    ra.store(stats, at, a.n_paths + i);
    if (var_T) var_T[a.n_paths + i] = sa.v;
  }
}

}  // namespace

QeArgs bates_launch_args(const hh_model& m, const hh_config& c, const hh_qe& qe, const hh_jump& jump) {
  const double r_c = m.r_drift - merton_compensator(jump);  // λ = 0: r_c == r, qe_launch_args' constants bit for bit
  return qe_args(m.kappa, m.theta, m.sigma, m.rho, r_c, m.T / (double)c.n_steps, qe.psi_c);
}

int launch_bates_stats(const hh_model& m, const hh_config& c, const hh_qe& qe, const hh_jump& jump,
                       const uint64_t* seeds_dev, uint32_t monitor_every, bool include_start, double* stats,
                       double* var_T, hipStream_t s) {
  DevicePtrs p{};
  p.seeds = seeds_dev;
  const SimArgs<0> a = make_args0(m, c, p);
  const QeArgs q = bates_launch_args(m, c, qe, jump);
  const JumpArgs j = jump_args(jump, m.T / (double)c.n_steps);
  const dim3 g((unsigned)((c.n_paths + 255) / 256)), blk(256);
  const bool anti = c.antithetic != 0, mart = qe.martingale != 0;
  auto kernel = anti ? (mart ? bates_stats_kernel<true, true> : bates_stats_kernel<true, false>)
                     : (mart ? bates_stats_kernel<false, true> : bates_stats_kernel<false, false>);
  hipLaunchKernelGGL(kernel, g, blk, 0, s, a, q, j, m.S0, monitor_every, (int)include_start, stats, var_T);
  return (int)hipGetLastError();
}

}  // namespace hh
