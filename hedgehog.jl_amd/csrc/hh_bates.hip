// Bates (1996) for gfx950 (wave64, fp64 VALU): Heston variance by the quadratic-exponential step plus Merton jumps in
// log S (include/hedgehog_mc.h, "Bates (1996): Heston variance with Merton jumps" — the step, the draws and the
// host-formed constants are stated there in full).  The step's arithmetic is hh_qe.h's, the jump count and the jump sum
// are hh_jump.h's; both are shared with host programs.
//
//   bates_stats_kernel<ANTI, MART>  qe_stats_kernel's form — one trajectory per lane and its mirror in the same lane, the
//                                   shared monitor (hh_path_stats.h) around qe_pair_step (hh_qe.h), the same five rows
//                                   and var_T — with jump_stats_kernel's two additions per step k (hh_jump.h): the jump
//                                   count N_k from the uniform of block (k >> 1, 0, 0, kDomJump) and jump_step, after
//                                   the QE step and before the date.  Its output goes through path_payoff_kernel
//                                   untouched.
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

// Sink (hh_path_stats.h): Monitor, the five statistics — or DateRows, the date-row form: `stats` is then the grid
// [n_steps/monitor_every + 1][n_total], row j the spot after step j·monitor_every, and include_start is not read.  The
// walk, its draws and its constants are stated here once for both.
// The date-row form writes spots alone: no variance rows, var_T is not read.  StateRows: `stats` is the state rows
// [n_steps/monitor_every + 1][2][n_total], (x, v) after step j·monitor_every; var_T is not read (it is the last v row).
template <bool ANTI, bool MART, class Sink = Monitor<ANTI>>
__global__ __launch_bounds__(256) void bates_stats_kernel(const SimArgs<0> a, const QeArgs q, const JumpArgs j,
                                                          const double S0, const uint32_t monitor_every,
                                                          const int include_start, double* __restrict__ stats,
                                                          double* __restrict__ var_T) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  QeState st{a.x0.v, a.v0.v}, sa{a.x0.v, a.v0.v};
  Sink mon(monitor_every, include_start);
  mon.bind(stats, i, a.n_paths);
  if constexpr (Sink::kStates) mon.start(a.x0.v, a.v0.v);
  else mon.start(S0, a.x0.v);
  const uint64_t key = a.seeds[i];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  JumpUniforms ju;
  for (uint32_t k = 0; k < n_steps; ++k) {
    qe_pair_step<ANTI, MART>(st, sa, q, key, k);
    const double uj = (k & 1u) == 0u ? ju.even(k >> 1, k0, k1) : ju.odd();
    jump_step<ANTI>(j, key, k, uj, st.x, sa.x);
    if constexpr (Sink::kStates) mon.date(st.x, sa.x, st.v, sa.v);
    else mon.date(st.x, sa.x);
  }
  if constexpr (Sink::kStats) {
    // each member's rows, then its var_T (Monitor::store writes the rows alone)
    mon.r.store(stats, at, i);
    if (var_T) var_T[i] = st.v;
    if constexpr (ANTI) {
      mon.ra.store(stats, at, a.n_paths + i);
      if (var_T) var_T[a.n_paths + i] = sa.v;
    }
  }
}

}  // namespace

QeArgs bates_launch_args(const hh_model& m, const hh_config& c, const hh_qe& qe, const hh_jump& jump) {
  const double r_c = m.r_drift - merton_compensator(jump);  // λ = 0: r_c == r, qe_launch_args' constants bit for bit
  return qe_args(m.kappa, m.theta, m.sigma, m.rho, r_c, m.T / (double)c.n_steps, qe.psi_c);
}

int launch_bates_stats(const hh_model& m, const hh_config& c, const hh_qe& qe, const hh_jump& jump,
                       const uint64_t* seeds_dev, uint32_t monitor_every, bool include_start, double* stats,
                       double* var_T, hipStream_t s, bool date_rows, bool state_rows) {
  const StatsLaunch l(m, c, seeds_dev);
  const QeArgs q = bates_launch_args(m, c, qe, jump);
  const JumpArgs j = jump_args(jump, m.T / (double)c.n_steps);
  const bool anti = c.antithetic != 0, mart = qe.martingale != 0;
  auto kernel = anti ? (mart ? bates_stats_kernel<true, true> : bates_stats_kernel<true, false>)
                     : (mart ? bates_stats_kernel<false, true> : bates_stats_kernel<false, false>);
  if (date_rows)
    kernel = anti ? (mart ? bates_stats_kernel<true, true, DateRows<true>> : bates_stats_kernel<true, false, DateRows<true>>)
                  : (mart ? bates_stats_kernel<false, true, DateRows<false>> : bates_stats_kernel<false, false, DateRows<false>>);
  if (state_rows)
    kernel = anti ? (mart ? bates_stats_kernel<true, true, StateRows<true>> : bates_stats_kernel<true, false, StateRows<true>>)
                  : (mart ? bates_stats_kernel<false, true, StateRows<false>> : bates_stats_kernel<false, false, StateRows<false>>);
  hipLaunchKernelGGL(kernel, l.grid, l.block, 0, s, l.a, q, j, m.S0, monitor_every, (int)include_start, stats, var_T);
  return (int)hipGetLastError();
}

}  // namespace hh
