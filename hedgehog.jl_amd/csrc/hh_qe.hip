// Heston paths by Andersen's quadratic-exponential scheme for gfx950 (wave64, fp64 VALU): include/hedgehog_mc.h,
// "Heston paths by the quadratic-exponential scheme" — the step, the draws and the host-formed constants are stated
// there in full; the step's arithmetic lives in hh_qe.h, shared with a host program.
//
//   qe_stats_kernel<ANTI, MART>  path_stats_kernel's monitored form with the QE step in place of the Euler step: one
//                                trajectory per lane and its mirror in the same lane, the shared monitor
//                                (hh_path_stats.h) around qe_pair_step (hh_qe.h), the same five rows.  Its output goes
//                                through path_payoff_kernel untouched.  var_T (nullable): the variance at expiry of
//                                each member.
//
// The constants travel in QeArgs beside SimArgs<0>, whose layout stays as it is.  Every loop is bounded by n_steps; none
// by data.
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
__global__ __launch_bounds__(256) void qe_stats_kernel(const SimArgs<0> a, const QeArgs q, const double S0,
                                                       const uint32_t monitor_every, const int include_start,
                                                       double* __restrict__ stats, double* __restrict__ var_T) {
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
  for (uint32_t k = 0; k < n_steps; ++k) {
    qe_pair_step<ANTI, MART>(st, sa, q, key, k);
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

QeArgs qe_launch_args(const hh_model& m, const hh_config& c, const hh_qe& qe) {
  return qe_args(m.kappa, m.theta, m.sigma, m.rho, m.r_drift, m.T / (double)c.n_steps, qe.psi_c);
}

int launch_qe_stats(const hh_model& m, const hh_config& c, const hh_qe& qe, const uint64_t* seeds_dev,
                    uint32_t monitor_every, bool include_start, double* stats, double* var_T, hipStream_t s,
                    bool date_rows, bool state_rows) {
  const StatsLaunch l(m, c, seeds_dev);
  const QeArgs q = qe_launch_args(m, c, qe);
  const bool anti = c.antithetic != 0, mart = qe.martingale != 0;
  auto kernel = anti ? (mart ? qe_stats_kernel<true, true> : qe_stats_kernel<true, false>)
                     : (mart ? qe_stats_kernel<false, true> : qe_stats_kernel<false, false>);
  if (date_rows)
    kernel = anti ? (mart ? qe_stats_kernel<true, true, DateRows<true>> : qe_stats_kernel<true, false, DateRows<true>>)
                  : (mart ? qe_stats_kernel<false, true, DateRows<false>> : qe_stats_kernel<false, false, DateRows<false>>);
  if (state_rows)
    kernel = anti ? (mart ? qe_stats_kernel<true, true, StateRows<true>> : qe_stats_kernel<true, false, StateRows<true>>)
                  : (mart ? qe_stats_kernel<false, true, StateRows<false>> : qe_stats_kernel<false, false, StateRows<false>>);
  hipLaunchKernelGGL(kernel, l.grid, l.block, 0, s, l.a, q, m.S0, monitor_every, (int)include_start, stats, var_T);
  return (int)hipGetLastError();
}

}  // namespace hh
