// Merton (1976) jump diffusion for gfx950 (wave64, fp64 VALU): lognormal dynamics plus a compound Poisson sum of normal
// jumps in log S (include/hedgehog_mc.h, "Merton (1976) jump diffusion" — the draws and formulas are stated there in
// full).  Two kernels:
//
//   merton_exact_kernel  the terminal law: one normal for the diffusion, one jump count by inversion (hh_jump.h), one
//                        normal for the whole jump sum; payoff and sums as exact_gbm_kernel's (finish_path);
//   jump_stats_kernel    path_stats_kernel's lognormal form — the same increments and step around the shared monitor
//                        (hh_path_stats.h) — with a jump count per step and, on the rare lane that has one, a jump
//                        (hh_jump.h: jump_step, JumpUniforms).  Its output goes through path_payoff_kernel untouched.
//
// The jump parameters travel in JumpArgs beside SimArgs<0>, whose layout stays as it is.  Every loop is bounded by
// n_steps, the per-lane trajectory count or HH_JUMP_MAX_COUNT; none by data.  The search of the inversion and the
// N > 0 branch diverge: at λ·dt ≪ 1 nearly every lane leaves the search at n = 0 and the jump's Philox block is drawn
// by the rare lane only.
#include <cmath>

#include "hh_jump.h"
#include "hh_path_stats.h"
#include "hh_sim.h"

namespace hh {
namespace {

// ------------------------------------------------------------------------------------------
// terminal law
// ------------------------------------------------------------------------------------------
// Trajectory g = path_offset + i of the ONE stream keyed by seeds[0]: block (lo32 g, hi32 g, 0, kDomJump) gives z1, z2,
// block (lo32 g, hi32 g, 1, kDomJump) the uniform of the jump count.  A lane takes kMertonPerLane trajectories, 256
// apart (a wave's samples are contiguous), whatever the call: the draws go by global index, the records by n_paths.
template <bool ANTI>
__global__ __launch_bounds__(kTile) void merton_exact_kernel(const SimArgs<0> a, const JumpArgs j) {
  const uint32_t chunk = blockIdx.x;
  double acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = 0.0;
  const uint64_t key = a.seeds[0];
  for (int t = 0; t < kMertonPerLane; ++t) {
    const uint64_t path = ((uint64_t)chunk * kMertonPerLane + t) * kTile + threadIdx.x;
    if (path >= a.n_paths) break;  // later t: larger still
    const uint64_t g = a.path_offset + path;
    const uint32_t glo = (uint32_t)g, ghi = (uint32_t)(g >> 32);
    double z1, z2;
    normal_pair(key, glo, ghi, 0u, kDomJump, z1, z2);
    const Philox4 b = philox4x32_10(glo, ghi, 1u, kDomJump, (uint32_t)key, (uint32_t)(key >> 32));
    const uint32_t N = poisson_inverse(u01_fast(b.c0, b.c1), j.mean, j.p0);
    GbmModel<0>::State st, sa;
    st.x.v = fma(a.law_sd.v, z1, a.law_mu.v);
    if constexpr (ANTI) sa.x.v = fma(a.law_sd.v, -z1, a.law_mu.v);
    if (N > 0u) {
      st.x.v = st.x.v + jump_sum(j, N, z2);
      if constexpr (ANTI) sa.x.v = sa.x.v + jump_sum(j, N, -z2);
    }
    finish_path<0, ANTI>(st, sa, a, path, acc);
  }
  block_reduce_store<4, kTile / 64, 2>(acc, a.records + (size_t)chunk * kRecStride);
}

// ------------------------------------------------------------------------------------------
// path form: the five monitored statistics under jumps
// ------------------------------------------------------------------------------------------
// path_stats_kernel<GbmModel<0>, ANTI, false> with two additions per step k: the jump count N_k from the uniform of
// block (k >> 1, 0, 0, kDomJump) — words 0, 1 for an even step, 2, 3 for an odd one (JumpUniforms) — and jump_step,
// after the step and before the date.  The mirror takes -dW, the same N_k and -z.  a.gdrift carries the compensator;
// with mean = 0 no lane ever jumps and every operation left is path_stats_kernel's.
// Sink (hh_path_stats.h): Monitor, the five statistics — or DateRows, the date-row form: `stats` is then the grid
// [n_steps/monitor_every + 1][n_total], row j the spot after step j·monitor_every, and include_start is not read.  The
// walk, its draws and its constants are stated here once for both.
template <bool ANTI, class Sink = Monitor<ANTI>>
__global__ __launch_bounds__(256) void jump_stats_kernel(const SimArgs<0> a, const JumpArgs j, const double S0,
                                                         const uint32_t monitor_every, const int include_start,
                                                         double* __restrict__ stats) {
  using M = GbmModel<0>;
  using State = typename M::State;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  State st, sa;
  M::init(st, a);
  if constexpr (ANTI) M::init(sa, a);
  Sink mon(monitor_every, include_start);
  mon.bind(stats, i, a.n_paths);
  mon.start(S0, a.x0.v);
  const uint64_t key = a.seeds[i];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  auto advance = [&](uint32_t k, double dW, double u) {
    M::step(st, a, dW, 0.0);
    if constexpr (ANTI) M::step(sa, a, -dW, 0.0);
    jump_step<ANTI>(j, key, k, u, st.x.v, sa.x.v);
    mon.date(st.x.v, sa.x.v);
  };
  // scalar noise: one Philox block feeds two consecutive steps, and so does one block of jump uniforms
  JumpUniforms ju;
  for (uint32_t s = 0; s < n_steps; s += 2) {
    double z1, z2;
    euler_scalar_normals(key, s >> 1, z1, z2);
    advance(s, a.sqrt_dt * z1, ju.even(s >> 1, k0, k1));
    if (s + 1 < n_steps) advance(s + 1, a.sqrt_dt * z2, ju.odd());
  }
  mon.store(stats, at, i, a.n_paths);
}

}  // namespace

int launch_merton_exact(const hh_model& m, const hh_config& c, const hh_jump& jump, const DevicePtrs& p, hipStream_t s) {
  SimArgs<0> a = make_args0(m, c, p);
  // m_T = log S0 + ((r − σ²/2) − λκ̄)·T: the lognormal law's mean with the compensated drift, ·T as it stands
  a.law_mu.v = a.x0.v + (a.gdrift.v - merton_compensator(jump)) * m.T;
  a.n_tiles = merton_records(c.n_paths);
  a.accum = nullptr;
  const JumpArgs j = jump_args(jump, m.T);
  auto kernel = c.antithetic ? merton_exact_kernel<true> : merton_exact_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(a.n_tiles), dim3(kTile), 0, s, a, j);
  return (int)hipGetLastError();
}

int launch_jump_stats(const hh_model& m, const hh_config& c, const hh_jump& jump, const uint64_t* seeds_dev,
                      uint32_t monitor_every, bool include_start, double* stats, hipStream_t s, bool date_rows) {
  StatsLaunch l(m, c, seeds_dev);
  l.a.gdrift.v = l.a.gdrift.v - merton_compensator(jump);  // (r − σ²/2) − λκ̄, in that order: λ = 0 leaves the lognormal drift
  const JumpArgs j = jump_args(jump, l.a.dt);
  auto kernel = c.antithetic ? (date_rows ? jump_stats_kernel<true, DateRows<true>> : jump_stats_kernel<true>)
                             : (date_rows ? jump_stats_kernel<false, DateRows<false>> : jump_stats_kernel<false>);
  hipLaunchKernelGGL(kernel, l.grid, l.block, 0, s, l.a, j, m.S0, monitor_every, (int)include_start, stats);
  return (int)hipGetLastError();
}

}  // namespace hh
