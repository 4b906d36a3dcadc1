// Several correlated lognormal assets for gfx950 (wave64, fp64 VALU): the five monitored statistics of
// path_stats_kernel (hh_path_stats.h: Running) for a scalar INDEX of d assets — a weighted sum, a geometric mean, the
// best or the worst of them (include/hedgehog_mc.h, "Several correlated lognormal assets" — the draws, the step and the
// index are stated there in full).  Its output goes through path_payoff_kernel untouched: every payoff kind prices on
// the index.
//
// One trajectory per lane, and its mirror in the same lane.  d, the index kind and the mirror are template
// parameters and every loop over assets is unrolled in full: the d log-states (2d with the mirror) and the d normals
// of a step are named registers — a per-thread array indexed at run time would go to scratch.  The Cholesky factor and
// the step's constants are formed on the host (hh_assets.h) and arrive by value: wave-uniform.  No LDS, no barriers;
// every loop is bounded by n_steps or by d.  index_of and step_assets are stated in hh_assets.h, for this unit's two kernels
// and for the induction that reads the state rows (hh_lsm_multi.hip).
#include <cmath>

#include "hh_assets.h"
#include "hh_path_stats.h"
#include "hh_sim.h"

namespace hh {
namespace {

// The dates, the first-term flag and the pair of Running objects are written out here as Monitor (hh_path_stats.h) writes
// them for the other four kernels of the family: on the monitor (the index from a callable, on a date only) 38 of the 64
// instantiations compiled to a prologue a few moves different from this text's, and timed against this text six of
// them missed the bar of the comparison (the appendix of profiles/path_family_refactor.txt).
template <int D, int KIND, bool ANTI>
__global__ __launch_bounds__(256) void assets_stats_kernel(const AssetArgs c, const uint64_t* __restrict__ seeds,
                                                           const uint64_t n_paths, const uint32_t n_steps,
                                                           const uint32_t monitor_every, const int include_start,
                                                           double* __restrict__ stats) {
  constexpr int H = (D + 1) / 2;  // Philox blocks, and Box–Muller pairs, of a step
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_paths) return;
  const PathStatsLayout at(n_paths, ANTI, HH_PATH_STATS);
  double x[D], xa[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = xa[k] = c.x0[k];
  Running r, ra;
  bool started = include_start != 0;
  if (started) {
    double I, xi;
    index_of<D, KIND>(c, x, I, xi);
    r.first(I, xi);
    if constexpr (ANTI) ra.first(I, xi);  // the mirror starts from the same states
  }
  const uint64_t key = seeds[i];
  uint32_t left = monitor_every;
  for (uint32_t s = 0; s < n_steps; ++s) {
    double z[2 * H];
#pragma unroll
    for (int h = 0; h < H; ++h) normal_pair(key, s, (uint32_t)h, 0u, kDomAssets, z[2 * h], z[2 * h + 1]);
    step_assets<D, false>(c, x, z);
    if constexpr (ANTI) step_assets<D, true>(c, xa, z);
    if (--left != 0u) continue;
    left = monitor_every;
    double I, xi;
    index_of<D, KIND>(c, x, I, xi);
    if (started) r.next(I, xi);
    else r.first(I, xi);
    if constexpr (ANTI) {
      index_of<D, KIND>(c, xa, I, xi);
      if (started) ra.next(I, xi);
      else ra.first(I, xi);
    }
    started = true;
  }
  r.store(stats, at, i);
  if constexpr (ANTI) ra.store(stats, at, n_paths + i);
}

using AssetsKernel = void (*)(const AssetArgs, const uint64_t*, const uint64_t, const uint32_t, const uint32_t, const int,
                              double*);

template <int D, int KIND>
AssetsKernel pick_member(bool anti) {
  return anti ? assets_stats_kernel<D, KIND, true> : assets_stats_kernel<D, KIND, false>;
}
template <int D>
AssetsKernel pick_kind(int kind, bool anti) {
  switch (kind) {
    case HH_INDEX_WEIGHTED_SUM: return pick_member<D, HH_INDEX_WEIGHTED_SUM>(anti);
    case HH_INDEX_GEOMETRIC: return pick_member<D, HH_INDEX_GEOMETRIC>(anti);
    case HH_INDEX_BEST_OF: return pick_member<D, HH_INDEX_BEST_OF>(anti);
    case HH_INDEX_WORST_OF: return pick_member<D, HH_INDEX_WORST_OF>(anti);
    default: return nullptr;
  }
}
AssetsKernel pick_kernel(uint32_t d, int kind, bool anti) {
  switch (d) {
    case 1: return pick_kind<1>(kind, anti);
    case 2: return pick_kind<2>(kind, anti);
    case 3: return pick_kind<3>(kind, anti);
    case 4: return pick_kind<4>(kind, anti);
    case 5: return pick_kind<5>(kind, anti);
    case 6: return pick_kind<6>(kind, anti);
    case 7: return pick_kind<7>(kind, anti);
    case 8: return pick_kind<8>(kind, anti);
    default: return nullptr;
  }
}

// The state rows of the same walk, for the several-variable induction (hh_lsm_multi.hip): assets_stats_kernel's draws,
// step and host-formed AssetArgs, no statistics.  On every exercise_every-th step the d log-states go out as the walk
// holds them (log w_i folded in under best-of and worst-of: AssetArgs::x0) into rows[date][asset][column], n_total
// columns, the mirror's into column n_paths + i — so index_of<D, KIND> on a stored row is the statistics kernel's (I, x)
// bit for bit, and the kernel does not depend on the index kind.  Row 0 is x0, plain stores; the later rows are written
// once and read far beyond what the caches hold: nontemporal stores, as DateRows'.  One lane writes one column: a wave's
// store is 512 contiguous bytes per date, asset and member.  The lane carries the address of its column in the next
// date's first row; the countdown is a uniform branch.
template <int D, bool ANTI>
__global__ __launch_bounds__(256) void assets_rows_kernel(const AssetArgs c, const uint64_t* __restrict__ seeds,
                                                          const uint64_t n_paths, const uint32_t n_steps,
                                                          const uint32_t exercise_every, double* __restrict__ rows) {
  constexpr int H = (D + 1) / 2;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_paths) return;
  const size_t n_total = (size_t)(ANTI ? 2 * n_paths : n_paths);
  double x[D], xa[D];
  double* next = rows + i;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[k] = xa[k] = c.x0[k];
    next[(size_t)k * n_total] = x[k];
    if constexpr (ANTI) next[(size_t)k * n_total + n_paths] = x[k];
  }
  next += (size_t)D * n_total;
  const uint64_t key = seeds[i];
  uint32_t left = exercise_every;
  for (uint32_t s = 0; s < n_steps; ++s) {
    double z[2 * H];
#pragma unroll
    for (int h = 0; h < H; ++h) normal_pair(key, s, (uint32_t)h, 0u, kDomAssets, z[2 * h], z[2 * h + 1]);
    step_assets<D, false>(c, x, z);
    if constexpr (ANTI) step_assets<D, true>(c, xa, z);
    if (--left != 0u) continue;
    left = exercise_every;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      __builtin_nontemporal_store(x[k], next + (size_t)k * n_total);
      if constexpr (ANTI) __builtin_nontemporal_store(xa[k], next + (size_t)k * n_total + n_paths);
    }
    next += (size_t)D * n_total;
  }
}

using RowsKernel = void (*)(const AssetArgs, const uint64_t*, const uint64_t, const uint32_t, const uint32_t, double*);

template <int D>
RowsKernel pick_rows_member(bool anti) {
  return anti ? assets_rows_kernel<D, true> : assets_rows_kernel<D, false>;
}
RowsKernel pick_rows_kernel(uint32_t d, bool anti) {
  switch (d) {
    case 1: return pick_rows_member<1>(anti);
    case 2: return pick_rows_member<2>(anti);
    case 3: return pick_rows_member<3>(anti);
    case 4: return pick_rows_member<4>(anti);
    case 5: return pick_rows_member<5>(anti);
    case 6: return pick_rows_member<6>(anti);
    case 7: return pick_rows_member<7>(anti);
    case 8: return pick_rows_member<8>(anti);
    default: return nullptr;
  }
}

}  // namespace

int launch_assets_stats(const hh_model& m, const hh_config& c, const hh_assets& assets, const uint64_t* seeds_dev,
                        uint32_t monitor_every, bool include_start, double* stats, hipStream_t s) {
  double L[kAssetsTri] = {};
  const AssetsKernel kernel = pick_kernel(assets.n_assets, assets.index_kind, c.antithetic != 0);
  if (!kernel || !cholesky(assets.corr, assets.n_assets, L)) return (int)hipErrorInvalidValue;  // the entry points check both
  const AssetArgs a = asset_args(assets, m.r_drift, m.T, c.n_steps, L);
  const StatsLaunch l(c);
  hipLaunchKernelGGL(kernel, l.grid, l.block, 0, s, a, seeds_dev, (uint64_t)c.n_paths, (uint32_t)c.n_steps, monitor_every,
                     (int)include_start, stats);
  return (int)hipGetLastError();
}

int launch_assets_rows(const hh_model& m, const hh_config& c, const hh_assets& assets, const uint64_t* seeds_dev,
                       uint32_t exercise_every, double* rows, hipStream_t s) {
  double L[kAssetsTri] = {};
  const RowsKernel kernel = pick_rows_kernel(assets.n_assets, c.antithetic != 0);
  if (!kernel || !cholesky(assets.corr, assets.n_assets, L)) return (int)hipErrorInvalidValue;  // the entry points check both
  const AssetArgs a = asset_args(assets, m.r_drift, m.T, c.n_steps, L);
  const StatsLaunch l(c);
  hipLaunchKernelGGL(kernel, l.grid, l.block, 0, s, a, seeds_dev, (uint64_t)c.n_paths, (uint32_t)c.n_steps, exercise_every,
                     rows);
  return (int)hipGetLastError();
}

}  // namespace hh
