// Local volatility for gfx950 (wave64, fp64 VALU): dS = r·S·dt + σ(t, S)·S·dW on a tabulated surface σ(t, log S)
// (include/hedgehog_mc.h, "Local volatility on a tabulated surface" — the lookup and the step are stated there in full;
// hh_localvol.h holds them).  One kernel:
//
//   localvol_stats_kernel  path_stats_kernel's lognormal form — the same increments, bridge draws, Monitor and Extremes
//                          (hh_path_stats.h) — whose step reads its σ from the surface: a bilinear gather per step and
//                          member from a copy of the whole table in LDS.  Its output goes through path_payoff_kernel
//                          untouched.
//
// The table (n_times·n_x doubles, at most HH_LV_MAX_NODES = 64 KiB) is dynamic LDS sized to the call, loaded once per
// workgroup by all 256 threads, then ONE barrier, then the step loop with none in it.  Row j_k and weight w_k of step k
// are the host's (localvol_row), read from two per-step arrays: uniform over the workgroup.  Every loop is bounded by
// n_steps or the table's size; none by data.  Every LDS index is i or i + 1 with i <= n_x − 2 in row j or j + 1 with
// j <= n_times − 2 (one row: row 0 alone): inside the table whatever x is.
#include "hh_localvol.h"
#include "hh_path_stats.h"
#include "hh_sim.h"

namespace hh {
namespace {

// One trajectory per lane (and its mirror, −dW on its own state and its own σ, in the same lane: column n_paths + i),
// after path_stats_kernel<GbmModel<0>, ANTI, BRIDGE>.  The lanes past n_paths take part in the table's load and in the
// barrier and leave only then.  BRIDGE: the σ of the step, frozen over it, is the bridge's coefficient (Extremes); the
// mirror takes the bridge draws swapped, as there.
// Sink (hh_path_stats.h): Monitor, the five statistics — or DateRows, the date-row form: `stats` is then the grid
// [n_steps/monitor_every + 1][n_total], row j the spot after step j·monitor_every, and include_start is not read.  The
// walk, its draws and its constants are stated here once for both.
template <bool ANTI, bool BRIDGE, class Sink = Monitor<ANTI>>
__global__ __launch_bounds__(256) void localvol_stats_kernel(const SimArgs<0> a, const LocalVolArgs lv, const double S0,
                                                             const uint32_t monitor_every, const int include_start,
                                                             double* __restrict__ stats) {
  static_assert(Sink::kStats || !BRIDGE, "the continuous extremes are statistics: no date-row form");
  extern __shared__ double tab[];
  const uint32_t n_nodes = lv.n_times * lv.n_x;
  for (uint32_t q = threadIdx.x; q < n_nodes; q += 256u) tab[q] = lv.vols[q];
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, BRIDGE ? HH_PATH_STATS_BRIDGE : HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  const bool two_rows = lv.n_times > 1u;
  double x = a.x0.v, xa = a.x0.v;
  Sink mon(monitor_every, include_start);
  mon.bind(stats, i, a.n_paths);
  mon.start(S0, a.x0.v);
  Extremes e, ea;
  if constexpr (BRIDGE) {
    e.first(a.x0.v);
    if constexpr (ANTI) ea.first(a.x0.v);
  }
  const uint64_t key = a.seeds[i];
  // step k: the σ of each member at its own state, the step, the extremes of bridge k, the date
  auto advance = [&](uint32_t k, double dW) {
    const double w = lv.step_w[k];
    const double* ra = tab + lv.step_row[k] * lv.n_x;
    const double* rb = ra + (two_rows ? lv.n_x : 0u);
    const double x0 = x, xa0 = xa;
    const double sg = localvol_sigma(ra, rb, two_rows, localvol_cell(x0, lv.x_lo, lv.inv_h, lv.n_x), w);
    x = localvol_step(x0, sg, a.r.v, a.dt, dW);
    double sga = 0.0;
    if constexpr (ANTI) {
      sga = localvol_sigma(ra, rb, two_rows, localvol_cell(xa0, lv.x_lo, lv.inv_h, lv.n_x), w);
      xa = localvol_step(xa0, sga, a.r.v, a.dt, -dW);
    }
    if constexpr (BRIDGE) {
      double L1, L2;
      euler_bridge_draws(key, k, L1, L2);
      e.next(x0, x, (sg * sg) * a.dt, L1, L2);
      if constexpr (ANTI) ea.next(xa0, xa, (sga * sga) * a.dt, L2, L1);
    }
    mon.date(x, xa);
  };
  // scalar noise: one Philox block feeds two consecutive steps
  for (uint32_t s = 0; s < n_steps; s += 2) {
    double z1, z2;
    euler_scalar_normals(key, s >> 1, z1, z2);
    advance(s, a.sqrt_dt * z1);
    if (s + 1 < n_steps) advance(s + 1, a.sqrt_dt * z2);
  }
  mon.store(stats, at, i, a.n_paths);
  if constexpr (BRIDGE) {
    e.store(stats, at, i);
    if constexpr (ANTI) ea.store(stats, at, a.n_paths + i);
  }
}

}  // namespace

int launch_localvol_stats(const hh_model& m, const hh_config& c, const LocalVolArgs& lv, const uint64_t* seeds_dev,
                          uint32_t monitor_every, bool include_start, bool bridge, double* stats, hipStream_t s,
                          bool date_rows) {
  const StatsLaunch l(m, c, seeds_dev);
  const size_t lds = (size_t)lv.n_times * lv.n_x * sizeof(double);  // <= HH_LV_MAX_NODES·8 = 64 KiB: the entry points check
  auto go = [&](auto anti, auto br) {
    hipLaunchKernelGGL((localvol_stats_kernel<decltype(anti)::value, decltype(br)::value>), l.grid, l.block, lds, s, l.a,
                       lv, m.S0, monitor_every, (int)include_start, stats);
  };
  auto with_form = [&](auto anti) {
    constexpr bool kAnti = decltype(anti)::value;
    if (date_rows)
      hipLaunchKernelGGL((localvol_stats_kernel<kAnti, false, DateRows<kAnti>>), l.grid, l.block, lds, s, l.a, lv, m.S0,
                         monitor_every, 1, stats);
    else if (bridge) go(anti, std::true_type{});
    else go(anti, std::false_type{});
  };
  if (c.antithetic) with_form(std::true_type{});
  else with_form(std::false_type{});
  return (int)hipGetLastError();
}

}  // namespace hh
