// Variance Gamma (Madan, Carr and Chang 1998) for gfx950 (wave64, fp64 VALU): a Brownian motion with drift run on a
// gamma clock (include/hedgehog_mc.h, "Variance Gamma" — the draws and formulas are stated there in full).  Two kernels:
//
//   vg_exact_kernel  the terminal law: one gamma variate of shape T/ν (hh_vg.h, gamma_mt) and one normal; payoff and
//                    sums as merton_exact_kernel's (finish_path);
//   vg_stats_kernel  the path form: one gamma variate of shape dt/ν per step and the lognormal statistics kernel's normal
//                    of that step, around the shared monitor (hh_path_stats.h).  Its output goes through
//                    path_payoff_kernel untouched.
//
// The sampler's parameters travel in VgArgs beside SimArgs<0>, whose layout stays as it is.  Every loop is bounded by
// n_steps, the per-lane trajectory count or HH_VG_MAX_ATTEMPTS; none by data.
//
// The rejection loop on the wave: a lane accepts an attempt with probability >= 0.95, so all 64 lanes of a wave are done
// after the first round only 4 % of the time and a wave runs 2-3 rounds per variate — the lanes that have accepted wait,
// masked off.  What a round costs is therefore what the SLOWEST path through an attempt costs (two Philox blocks, the
// Box–Muller pair, two logarithms and, boosted, a third one and an exponential): a squeeze test that spares a lane its
// logarithms spares the wave nothing and is not made.  The loop carries no array and no address: no scratch, no LDS.
#include <cmath>

#include "hh_path_stats.h"
#include "hh_sim.h"
#include "hh_vg.h"

namespace hh {
namespace {

// The draws of attempt t under one key (k0, k1).  Terminal law, (w0, w1) = the trajectory's global index: block
// (w0, w1, 2t, kDomVg) gives z, the first normal of its Box–Muller pair; block (w0, w1, 2t + 1, kDomVg) gives U from
// output words 0, 1 and U′ from words 2, 3.
struct VgLawDraws {
  uint32_t w0, w1, k0, k1;
  __device__ __forceinline__ VgDraws attempt(uint32_t t) const {
    VgDraws w;
    double unused;
    normal_pair(philox4x32_10(w0, w1, 2u * t, kDomVg, k0, k1), w.z, unused);
    const Philox4 b = philox4x32_10(w0, w1, 2u * t + 1u, kDomVg, k0, k1);
    w.u = u01_fast(b.c0, b.c1);
    w.u_boost = u01_fast(b.c2, b.c3);
    return w;
  }
};
// Path form, step k: block (k, t, 0, kDomVg) gives z, block (k, t, 1, kDomVg) U and U′.
struct VgStepDraws {
  uint32_t k, k0, k1;
  __device__ __forceinline__ VgDraws attempt(uint32_t t) const {
    VgDraws w;
    double unused;
    normal_pair(philox4x32_10(k, t, 0u, kDomVg, k0, k1), w.z, unused);
    const Philox4 b = philox4x32_10(k, t, 1u, kDomVg, k0, k1);
    w.u = u01_fast(b.c0, b.c1);
    w.u_boost = u01_fast(b.c2, b.c3);
    return w;
  }
};

// ------------------------------------------------------------------------------------------
// terminal law
// ------------------------------------------------------------------------------------------
// Trajectory g = path_offset + i of the ONE stream keyed by seeds[0]: the gamma variate from the attempts' blocks
// (lo32 g, hi32 g, 2t | 2t + 1, kDomVg), the normal from block (lo32 g, hi32 g, 2·HH_VG_MAX_ATTEMPTS, kDomVg).  A lane
// takes kVgPerLane trajectories, 256 apart (a wave's samples are contiguous), whatever the call: the draws go by global
// index, the records by n_paths.
template <bool ANTI>
__global__ __launch_bounds__(kTile) void vg_exact_kernel(const SimArgs<0> a, const VgArgs v) {
  const uint32_t chunk = blockIdx.x;
  double acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = 0.0;
  const uint64_t key = a.seeds[0];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  for (int t = 0; t < kVgPerLane; ++t) {
    const uint64_t path = ((uint64_t)chunk * kVgPerLane + t) * kTile + threadIdx.x;
    if (path >= a.n_paths) break;  // later t: larger still
    const uint64_t g = a.path_offset + path;
    const uint32_t glo = (uint32_t)g, ghi = (uint32_t)(g >> 32);
    VgLawDraws src{glo, ghi, k0, k1};
    const double G = gamma_mt(v, src);
    double z, unused;
    normal_pair(key, glo, ghi, 2u * (uint32_t)HH_VG_MAX_ATTEMPTS, kDomVg, z, unused);
    GbmModel<0>::State st, sa;
    st.x.v = a.x0.v + vg_increment(v, a.sigma.v, G, z);
    if constexpr (ANTI) sa.x.v = a.x0.v + vg_increment(v, a.sigma.v, G, -z);
    finish_path<0, ANTI>(st, sa, a, path, acc);
  }
  block_reduce_store<4, kTile / 64, 2>(acc, a.records + (size_t)chunk * kRecStride);
}

// ------------------------------------------------------------------------------------------
// path form: the five monitored statistics on the gamma clock
// ------------------------------------------------------------------------------------------
// Trajectory i under seeds[i].  Step k: the gamma variate of shape dt/ν from VgStepDraws' blocks, the normal the
// lognormal path_stats_kernel draws for step k (euler_scalar_normals, domain 0: one block per two steps, an odd n_steps
// leaving the last block half read), x ← x + vg_increment, then the date.  The mirror takes the same variate and −z.
// Sink (hh_path_stats.h): Monitor, the five statistics — or DateRows, the date-row form: `stats` is then the grid
// [n_steps/monitor_every + 1][n_total], row j the spot after step j·monitor_every, and include_start is not read.  The
// walk, its draws and its constants are stated here once for both.
template <bool ANTI, class Sink = Monitor<ANTI>>
__global__ __launch_bounds__(256) void vg_stats_kernel(const SimArgs<0> a, const VgArgs v, const double S0,
                                                       const uint32_t monitor_every, const int include_start,
                                                       double* __restrict__ stats) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  double x = a.x0.v, xa = a.x0.v;
  Sink mon(monitor_every, include_start);
  mon.bind(stats, i, a.n_paths);
  mon.start(S0, a.x0.v);
  const uint64_t key = a.seeds[i];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  auto advance = [&](uint32_t k, double z) {
    VgStepDraws src{k, k0, k1};
    const double G = gamma_mt(v, src);
    x = x + vg_increment(v, a.sigma.v, G, z);
    if constexpr (ANTI) xa = xa + vg_increment(v, a.sigma.v, G, -z);
    mon.date(x, xa);
  };
  for (uint32_t s = 0; s < n_steps; s += 2) {
    double z1, z2;
    euler_scalar_normals(key, s >> 1, z1, z2);
    advance(s, z1);
    if (s + 1 < n_steps) advance(s + 1, z2);
  }
  mon.store(stats, at, i, a.n_paths);
}

}  // namespace

int launch_vg_exact(const hh_model& m, const hh_config& c, const hh_vg& vg, const DevicePtrs& p, hipStream_t s) {
  SimArgs<0> a = make_args0(m, c, p);
  a.n_tiles = vg_records(c.n_paths);
  a.accum = nullptr;
  const VgArgs v = vg_args(m.sigma, m.r_drift, vg, m.T);
  auto kernel = c.antithetic ? vg_exact_kernel<true> : vg_exact_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(a.n_tiles), dim3(kTile), 0, s, a, v);
  return (int)hipGetLastError();
}

int launch_vg_stats(const hh_model& m, const hh_config& c, const hh_vg& vg, const uint64_t* seeds_dev,
                    uint32_t monitor_every, bool include_start, double* stats, hipStream_t s, bool date_rows) {
  StatsLaunch l(m, c, seeds_dev);
  const VgArgs v = vg_args(m.sigma, m.r_drift, vg, l.a.dt);
  auto kernel = c.antithetic ? (date_rows ? vg_stats_kernel<true, DateRows<true>> : vg_stats_kernel<true>)
                             : (date_rows ? vg_stats_kernel<false, DateRows<false>> : vg_stats_kernel<false>);
  hipLaunchKernelGGL(kernel, l.grid, l.block, 0, s, l.a, v, m.S0, monitor_every, (int)include_start, stats);
  return (int)hipGetLastError();
}

}  // namespace hh
