// Path-dependent payoffs on Euler–Maruyama paths for gfx950: arithmetic / geometric Asian, barrier (on the simulation's
// dates, or continuously monitored by Brownian bridge), lookback, digital (include/hedgehog_mc.h, "Path-dependent
// payoffs").  Two kernels:
//
//   path_stats_kernel   simulates the trajectories of euler_kernel / euler_grid_kernel — the draws, the correlation
//                       and the step are hh_sim.h's, so every state is theirs bit for bit — and keeps, instead of a
//                       grid, HH_PATH_STATS running numbers per trajectory over the monitoring dates — and, in its
//                       bridge form, the maximum and minimum of the scheme's continuous interpolation as well;
//   path_payoff_kernel  evaluates any number of payoffs on those numbers, as basket_payoff_kernel evaluates strikes
//                       on terminal samples, and leaves one record of sums per payoff and chunk.
//
// The 40 bytes per trajectory that go through memory between the two are about 1 % of the simulation's time at
// 252 steps; in exchange one simulation serves every payoff of a call and the caller can have the statistics.
// Their pathwise-derivative siblings (include/hedgehog_mc.h, "Pathwise derivatives of path-dependent payoffs"; DESIGN
// §5.21): path_tangent_kernel walks the same trajectories on dual states and keeps the tangent of every statistic along
// the carried basis slots, path_payoff_tangent_kernel evaluates the Lipschitz payoffs and their derivatives on them.
#include "hh_path_stats.h"  // Monitor: the five statistics and their dates, shared by the family; Extremes
#include "hh_sim.h"

namespace hh {
namespace {

// One trajectory per lane (and its mirror, -dW, in the same lane: column n_paths + i), GENERATE noise, after
// euler_grid_kernel.  The monitoring dates are the steps monitor_every, 2·monitor_every, …, n_steps — monitor_every
// divides n_steps, so the last step is one, and S = exp(x) is formed there only, as euler_grid_kernel's `put` forms
// it — and step 0 (S0, log S0: the grid's row 0) when include_start: Monitor (hh_path_stats.h).  No LDS.
// BRIDGE: rows HH_STAT_CMAX_S, HH_STAT_CMIN_S as well (Extremes), over ALL steps whatever monitor_every; one more Philox
// block and two logarithms per step (euler_bridge_draws), shared with the mirror: -dW has the negated bridge, the
// excess of its maximum is the excess of the original's minimum, so the mirror's maximum takes L2 and its minimum L1.
// The trajectory and the five statistics are the other form's, operation for operation.
// Sink (hh_path_stats.h): Monitor, the five statistics — or DateRows, the date-row form: `stats` is then the grid
// [n_steps/monitor_every + 1][n_total], row j the spot after step j·monitor_every, and include_start is not read.  The
// walk, its draws and its constants are stated here once for both.
// At monitor_every = 1 the date rows are euler_grid_kernel's spot grid bit for bit.
// StateRows (HestonModel alone: the walk that holds a variance): `stats` is the state rows [n_steps/monitor_every + 1][2]
// [n_total], (x, v) after step j·monitor_every as the step leaves them — at monitor_every = 1 euler_grid_kernel's log
// states and its variance grid bit for bit.
template <class M, bool ANTI, bool BRIDGE, class Sink = Monitor<ANTI>>
__global__ __launch_bounds__(256) void path_stats_kernel(const SimArgs<0> a, const double S0,
                                                         const uint32_t monitor_every, const int include_start,
                                                         double* __restrict__ stats) {
  static_assert(Sink::kStats || !BRIDGE, "the continuous extremes are statistics: no date-row form");
  static_assert(!Sink::kStates || M::NCOMP == 2, "state rows need a walk that holds a variance");
  using State = typename M::State;
  constexpr int NC = M::NCOMP;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, BRIDGE ? HH_PATH_STATS_BRIDGE : HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  State st, sa;
  M::init(st, a);
  if constexpr (ANTI) M::init(sa, a);
  Sink mon(monitor_every, include_start);
  mon.bind(stats, i, a.n_paths);
  if constexpr (Sink::kStates) mon.start(a.x0.v, a.v0.v);
  else mon.start(S0, a.x0.v);
  Extremes e, ea;
  if constexpr (BRIDGE) {
    e.first(a.x0.v);
    if constexpr (ANTI) ea.first(a.x0.v);
  }
  const uint64_t key = a.seeds[i];  // montecarlo.jl:331
  // step k: the trajectory and its mirror (montecarlo.jl:258: -W), the extremes of bridge k, the date
  auto advance = [&](uint32_t k, double d1, double d2) {
    if constexpr (BRIDGE) {
      const double x0 = st.x.v;
      double xa0 = 0.0, g, ga = 0.0;
      if constexpr (ANTI) xa0 = sa.x.v;
      M::step(st, a, d1, d2, g);
      if constexpr (ANTI) M::step(sa, a, -d1, -d2, ga);
      double L1, L2;
      euler_bridge_draws(key, k, L1, L2);
      e.next(x0, st.x.v, (g * g) * a.dt, L1, L2);
      if constexpr (ANTI) ea.next(xa0, sa.x.v, (ga * ga) * a.dt, L2, L1);
    } else {
      M::step(st, a, d1, d2);
      if constexpr (ANTI) M::step(sa, a, -d1, -d2);
    }
    if constexpr (Sink::kStates) mon.date(st.x.v, sa.x.v, st.v.v, sa.v.v);
    else mon.date(st.x.v, sa.x.v);
  };
  if constexpr (NC == 2) {
    for (uint32_t s = 0; s < n_steps; ++s) {
      double d1, d2;
      euler_pair_increments(key, s, a, d1, d2);
      advance(s, d1, d2);
    }
  } else {
    // scalar noise: one Philox block feeds two consecutive steps
    for (uint32_t s = 0; s < n_steps; s += 2) {
      double z1, z2;
      euler_scalar_normals(key, s >> 1, z1, z2);
      advance(s, a.sqrt_dt * z1, 0.0);
      if (s + 1 < n_steps) advance(s + 1, a.sqrt_dt * z2, 0.0);
    }
  }
  mon.store(stats, at, i, a.n_paths);
  if constexpr (BRIDGE) {
    e.store(stats, at, i);
    if constexpr (ANTI) ea.store(stats, at, a.n_paths + i);
  }
}

// path_stats_kernel's monitored (non-bridge) walk, statement for statement, on dual states: M = GbmModel<P> or
// HestonModel<P, SPLIT> propagates the tangents along the P carried basis slots of `a` (make_basis_args: a unit seed on
// each carried parameter) through its fused per-step map, and TangentMonitor keeps the statistics with their tangents.
// The draws, the mirror on −dW and the Philox pairing of scalar noise are that kernel's: rows 0-4 are its rows bit for
// bit.  P = 0: no carried slot — the eight value and date rows alone.  PathTangentLayout(n_paths, ANTI, P).  No LDS.
template <class M, int P, bool ANTI>
__global__ __launch_bounds__(256) void path_tangent_kernel(const SimArgs<P> a, const double S0,
                                                           const uint32_t monitor_every, const int include_start,
                                                           double* __restrict__ rows) {
  using State = typename M::State;
  constexpr int NC = M::NCOMP;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathTangentLayout at(a.n_paths, ANTI, P);
  const uint32_t n_steps = a.n_steps;
  State st, sa;
  M::init(st, a);
  if constexpr (ANTI) M::init(sa, a);
  TangentMonitor<P, ANTI> mon(monitor_every, include_start);
  mon.start(S0, a.x0.v);
  const uint64_t key = a.seeds[i];  // montecarlo.jl:331
  auto advance = [&](double d1, double d2) {
    M::step(st, a, d1, d2);
    if constexpr (ANTI) M::step(sa, a, -d1, -d2);
    mon.date(st.x, sa.x);
  };
  if constexpr (NC == 2) {
    for (uint32_t s = 0; s < n_steps; ++s) {
      double d1, d2;
      euler_pair_increments(key, s, a, d1, d2);
      advance(d1, d2);
    }
  } else {
    // scalar noise: one Philox block feeds two consecutive steps
    for (uint32_t s = 0; s < n_steps; s += 2) {
      double z1, z2;
      euler_scalar_normals(key, s >> 1, z1, z2);
      advance(a.sqrt_dt * z1, 0.0);
      if (s + 1 < n_steps) advance(a.sqrt_dt * z2, 0.0);
    }
  }
  mon.store(rows, at, i, a.n_paths);
}

// ------------------------------------------------------------------------------------------
// payoffs on the statistics
// ------------------------------------------------------------------------------------------

constexpr int kPathKB = 4;  // payoffs a workgroup evaluates on each trajectory it loads

// q is the same for every lane of the workgroup (scalar registers): the switch is a scalar branch
__device__ __forceinline__ double path_payoff_of(const hh_path_payoff& q, const double (&t)[HH_PATH_STATS],
                                                 double n_mon) {
  const double S_T = t[HH_STAT_S_T];
  const double mT = q.cp * (S_T - q.strike);
  const double van = mT > 0.0 ? mT : 0.0;
  switch (q.kind) {
    case HH_PAYOFF_ASIAN_ARITH: {
      const double m = q.cp * (t[HH_STAT_SUM_S] / n_mon - q.strike);
      return m > 0.0 ? m : 0.0;
    }
    case HH_PAYOFF_ASIAN_GEOM: {
      const double m = q.cp * (exp(t[HH_STAT_SUM_X] / n_mon) - q.strike);
      return m > 0.0 ? m : 0.0;
    }
    case HH_PAYOFF_BARRIER: {
      const bool up = q.barrier_type == HH_BARRIER_UP_OUT || q.barrier_type == HH_BARRIER_UP_IN;
      const bool out = q.barrier_type == HH_BARRIER_UP_OUT || q.barrier_type == HH_BARRIER_DOWN_OUT;
      const bool hit = up ? t[HH_STAT_MAX_S] >= q.barrier : t[HH_STAT_MIN_S] <= q.barrier;
      return hit == out ? q.rebate : van;  // knock-out: hit ? rebate : van;  knock-in: hit ? van : rebate
    }
    case HH_PAYOFF_LOOKBACK_FLOAT: return q.cp > 0.0 ? S_T - t[HH_STAT_MIN_S] : t[HH_STAT_MAX_S] - S_T;
    case HH_PAYOFF_LOOKBACK_FIXED: {
      const double m = q.cp > 0.0 ? t[HH_STAT_MAX_S] - q.strike : q.strike - t[HH_STAT_MIN_S];
      return m > 0.0 ? m : 0.0;
    }
    case HH_PAYOFF_DIGITAL_CASH: return mT > 0.0 ? q.cash : 0.0;
    case HH_PAYOFF_DIGITAL_ASSET: return mT > 0.0 ? S_T : 0.0;
    default: return van;  // HH_PAYOFF_VANILLA (the entry point admits no other kind)
  }
}

// After basket_payoff_kernel, with its block -> (chunk, payoff group) map (chunk c on XCD c mod 8 whatever the group,
// so each XCD's L2 holds one eighth of the statistics for all payoffs): a workgroup loads the five statistics of a
// trajectory (and of its mirror) once and evaluates every payoff of its group on them from registers.  Each payoff
// keeps its own accumulators, lane order and record: its sums are those of a one-payoff launch bit for bit.
// b.extremes (uniform) says which rows a payoff's MAX / MIN are: the monitored ones, or — HH_EXTREMES_BRIDGE, a
// seven-row buffer — the continuous ones, loaded into the same two slots; nothing else differs between the modes.
__global__ __launch_bounds__(256) void path_payoff_kernel(const PathPayoffArgs b, const uint32_t n_payoffs) {
  const uint32_t per_xcd = (b.n_chunks + 7u) / 8u;  // chunks an XCD owns
  const uint32_t xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
  const uint32_t grp = idx / per_xcd, chunk = (idx % per_xcd) * 8u + xcd;
  if (chunk >= b.n_chunks) return;  // padding of the last group of eight
  const uint32_t k0 = grp * kPathKB;
  hh_path_payoff q[kPathKB];
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) q[g] = b.payoffs[min(k0 + g, n_payoffs - 1)];  // a short last group repeats its last payoff
  const bool anti = b.antithetic != 0;
  const bool cont = b.extremes == HH_EXTREMES_BRIDGE;
  const PathStatsLayout at(b.n_paths, anti, cont ? HH_PATH_STATS_BRIDGE : HH_PATH_STATS);
  const int row_max = cont ? HH_STAT_CMAX_S : HH_STAT_MAX_S, row_min = cont ? HH_STAT_CMIN_S : HH_STAT_MIN_S;
  double acc[kPathKB][2];
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) acc[g][0] = acc[g][1] = 0.0;
  const uint64_t i0 = (uint64_t)chunk * kBasketChunk;
  for (uint32_t j = threadIdx.x; j < (uint32_t)kBasketChunk; j += 256) {
    const uint64_t i = i0 + j;
    if (i >= b.n_paths) break;
    double t[HH_PATH_STATS], ta[HH_PATH_STATS];
#pragma unroll
    for (int s = 0; s < HH_PATH_STATS; ++s) {
      const int row = s == HH_STAT_MAX_S ? row_max : s == HH_STAT_MIN_S ? row_min : s;
      t[s] = b.stats[at.row(row) + i];
      ta[s] = anti ? b.stats[at.row(row) + b.n_paths + i] : 0.0;
    }
#pragma unroll
    for (int g = 0; g < kPathKB; ++g) {
      const bool live = k0 + g < n_payoffs;  // uniform over the workgroup
      double p = path_payoff_of(q[g], t, b.n_mon);
      if (b.values && live) b.values[(size_t)(k0 + g) * at.n_total + i] = p;
      if (anti) {
        const double pa = path_payoff_of(q[g], ta, b.n_mon);
        if (b.values && live) b.values[(size_t)(k0 + g) * at.n_total + b.n_paths + i] = pa;
        p = (p + pa) / 2;  // montecarlo.jl:431
      }
      acc[g][0] += p;
      acc[g][1] = fma(p, p, acc[g][1]);
    }
  }
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) {
    if (k0 + g >= n_payoffs) break;  // uniform over the workgroup
    if (g) __syncthreads();          // the reduction's LDS staging is reused
    block_reduce_store<2, 4, 0>(acc[g], b.records + ((size_t)(k0 + g) * b.n_chunks + chunk) * kRecStride);
  }
}

// ------------------------------------------------------------------------------------------
// payoffs and their pathwise derivatives on the tangent rows
// ------------------------------------------------------------------------------------------

// What a member's payoff derivative is made of.  Every rule of the header's table is linear in the tangents of the five
// statistics and in the strike seed:  ∂p_k = Σ_s c[s]·dStat_s[k] − cK·dK_k  (s: enum hh_path_tangent_row), and the
// tangent of a statistic is  Σ_b w[k][b]·(row s of slot b) + xd0_k·A_s + (dr_k·dt)·B_s  with the passive factors A_s, B_s
// of the header.  So per member and payoff seven numbers hold every direction:
//   basis[b] = Σ_s c[s]·(row s of slot b),   pa = Σ_s c[s]·A_s,   pb = Σ_s c[s]·B_s,   pk = cK
// and they are linear too: their sums over the trajectories are assembled into the directions once per record.
constexpr int kTanSums = kMaxBasis + 3;  // basis[0..3], pa, pb, pk

struct MemberRows {
  double t[HH_PATH_STATS];  // the five statistics
  double k_max, k_min, sum_ks;
  double d[kMaxBasis][HH_TANGENT_ROWS_PER_SLOT];
};

__device__ __forceinline__ void load_member(const PathTangentArgs& b, const PathTangentLayout& at, uint64_t col,
                                            MemberRows& r) {
#pragma unroll
  for (int s = 0; s < HH_PATH_STATS; ++s) r.t[s] = b.rows[at.row(s) + col];
  r.k_max = b.rows[at.row(HH_TANGENT_K_MAX) + col];
  r.k_min = b.rows[at.row(HH_TANGENT_K_MIN) + col];
  r.sum_ks = b.rows[at.row(HH_TANGENT_SUM_KS) + col];
#pragma unroll
  for (int j = 0; j < kMaxBasis; ++j)
#pragma unroll
    for (int s = 0; s < HH_TANGENT_ROWS_PER_SLOT; ++s)
      r.d[j][s] = j < b.n_active ? b.rows[at.slot_row(j, s) + col] : 0.0;  // uniform
}

// p: path_payoff_of's value, itm = p > 0 (every admitted kind's own comparison).  q is uniform: scalar branches.
__device__ __forceinline__ void payoff_tangent_of(const hh_path_payoff& q, const MemberRows& r, const PathTangentArgs& b,
                                                  double& p, double (&out)[kTanSums]) {
  p = path_payoff_of(q, r.t, b.n_mon);
  const double itm = p > 0.0 ? 1.0 : 0.0;
  double c[HH_TANGENT_ROWS_PER_SLOT] = {0.0, 0.0, 0.0, 0.0, 0.0}, cK = 0.0;
  switch (q.kind) {
    case HH_PAYOFF_ASIAN_ARITH:
      c[HH_TANGENT_DSUM_S] = itm * q.cp / b.n_mon;
      cK = itm * q.cp;
      break;
    case HH_PAYOFF_ASIAN_GEOM:
      c[HH_TANGENT_DSUM_X] = itm * q.cp * exp(r.t[HH_STAT_SUM_X] / b.n_mon) / b.n_mon;
      cK = itm * q.cp;
      break;
    case HH_PAYOFF_LOOKBACK_FLOAT:
      if (q.cp > 0.0) {
        c[HH_TANGENT_DS_T] = 1.0;
        c[HH_TANGENT_DMIN_S] = -1.0;
      } else {
        c[HH_TANGENT_DMAX_S] = 1.0;
        c[HH_TANGENT_DS_T] = -1.0;
      }
      break;
    case HH_PAYOFF_LOOKBACK_FIXED:
      if (q.cp > 0.0) {
        c[HH_TANGENT_DMAX_S] = itm;
        cK = itm;
      } else {
        c[HH_TANGENT_DMIN_S] = -itm;
        cK = -itm;
      }
      break;
    default:  // HH_PAYOFF_VANILLA (the entry point admits no other kind)
      c[HH_TANGENT_DS_T] = itm * q.cp;
      cK = itm * q.cp;
      break;
  }
  const double A[HH_TANGENT_ROWS_PER_SLOT] = {r.t[HH_STAT_SUM_S], b.n_mon, r.t[HH_STAT_MAX_S], r.t[HH_STAT_MIN_S],
                                              r.t[HH_STAT_S_T]};
  const double B[HH_TANGENT_ROWS_PER_SLOT] = {r.sum_ks, b.sum_k, r.t[HH_STAT_MAX_S] * r.k_max,
                                              r.t[HH_STAT_MIN_S] * r.k_min, r.t[HH_STAT_S_T] * b.n_steps};
#pragma unroll
  for (int j = 0; j < kMaxBasis; ++j) {
    double v = 0.0;
#pragma unroll
    for (int s = 0; s < HH_TANGENT_ROWS_PER_SLOT; ++s) v = fma(c[s], r.d[j][s], v);
    out[j] = v;
  }
  double pa = 0.0, pb = 0.0;
#pragma unroll
  for (int s = 0; s < HH_TANGENT_ROWS_PER_SLOT; ++s) {
    pa = fma(c[s], A[s], pa);
    pb = fma(c[s], B[s], pb);
  }
  out[kMaxBasis] = pa;
  out[kMaxBasis + 1] = pb;
  out[kMaxBasis + 2] = cK;
}

// block_reduce_store<2, 4, 0>'s adds in its order for Σp, Σp² — the record's first two slots are path_payoff_kernel's
// bit for bit — and the same tree for the seven tangent sums, which thread 0 assembles into the n_partials directions:
// slot HH_ACC_DSUM + k = Σ_b w[k][b]·Σbasis[b] + xd0_k·Σpa + (dr_k·dt)·Σpb − dK_k·Σpk.
__device__ __forceinline__ void tangent_reduce_store(double (&acc)[2 + kTanSums], const PathTangentArgs& b,
                                                     double* __restrict__ rec) {
  constexpr int N = 2 + kTanSums;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, 64);
  }
  __shared__ double sm[4][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) sm[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      t[i] = sm[0][i];
#pragma unroll
      for (int w = 1; w < 4; ++w) t[i] += sm[w][i];
    }
#pragma unroll
    for (int i = 0; i < kRecStride; ++i) rec[i] = 0.0;
    rec[HH_ACC_SUM] = t[0];
    rec[HH_ACC_SUMSQ] = t[1];
    for (int k = 0; k < b.n_partials; ++k) {
      double d = 0.0;
#pragma unroll
      for (int j = 0; j < kMaxBasis; ++j) d = fma(b.w[k][j], t[2 + j], d);
      d = fma(b.xd0[k], t[2 + kMaxBasis], d);
      d = fma(b.dr[k] * b.dt, t[2 + kMaxBasis + 1], d);
      d = fma(-b.dK[k], t[2 + kMaxBasis + 2], d);
      rec[HH_ACC_DSUM + k] = d;
    }
  }
}

// path_payoff_kernel's block -> (chunk, payoff group) map, payoffs per load and lane order, on path_tangent_kernel's
// rows.  Each payoff keeps its own accumulators and record: its price sums are hh_mc_solve_path's bit for bit, whatever
// else is in the call.  Antithetic: the pair average of the payoff and of each of its seven tangent numbers.
__global__ __launch_bounds__(256) void path_payoff_tangent_kernel(const PathTangentArgs b, const uint32_t n_payoffs) {
  const uint32_t per_xcd = (b.n_chunks + 7u) / 8u;
  const uint32_t xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
  const uint32_t grp = idx / per_xcd, chunk = (idx % per_xcd) * 8u + xcd;
  if (chunk >= b.n_chunks) return;  // padding of the last group of eight
  const uint32_t k0 = grp * kPathKB;
  hh_path_payoff q[kPathKB];
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) q[g] = b.payoffs[min(k0 + g, n_payoffs - 1)];
  const bool anti = b.antithetic != 0;
  const PathTangentLayout at(b.n_paths, anti, b.n_active);
  double acc[kPathKB][2 + kTanSums];
#pragma unroll
  for (int g = 0; g < kPathKB; ++g)
#pragma unroll
    for (int s = 0; s < 2 + kTanSums; ++s) acc[g][s] = 0.0;
  const uint64_t i0 = (uint64_t)chunk * kBasketChunk;
  for (uint32_t j = threadIdx.x; j < (uint32_t)kBasketChunk; j += 256) {
    const uint64_t i = i0 + j;
    if (i >= b.n_paths) break;
    MemberRows r, ra;
    load_member(b, at, i, r);
    if (anti) load_member(b, at, b.n_paths + i, ra);
#pragma unroll
    for (int g = 0; g < kPathKB; ++g) {
      double p, d[kTanSums];
      payoff_tangent_of(q[g], r, b, p, d);
      if (anti) {
        double pa, da[kTanSums];
        payoff_tangent_of(q[g], ra, b, pa, da);
        p = (p + pa) / 2;  // montecarlo.jl:431
#pragma unroll
        for (int s = 0; s < kTanSums; ++s) d[s] = (d[s] + da[s]) / 2;
      }
      acc[g][0] += p;
      acc[g][1] = fma(p, p, acc[g][1]);
#pragma unroll
      for (int s = 0; s < kTanSums; ++s) acc[g][2 + s] += d[s];
    }
  }
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) {
    if (k0 + g >= n_payoffs) break;  // uniform over the workgroup
    if (g) __syncthreads();          // the reduction's LDS staging is reused
    tangent_reduce_store(acc[g], b, b.records + ((size_t)(k0 + g) * b.n_chunks + chunk) * kRecStride);
  }
}

// ------------------------------------------------------------------------------------------
// multilevel Monte Carlo: a fine and a coarse trajectory on the same draws
// ------------------------------------------------------------------------------------------

// One lane per trajectory, GENERATE noise, no LDS.  The lane carries the FINE trajectory of path_stats_kernel<M, false,
// false> — a.n_steps steps of a.dt, the same draws, steps and dates, so column i is that kernel's bit for bit — and a
// COARSE one of a.n_steps/2 steps of ac.dt = 2·a.dt (ac: make_args0 on the coarse grid, a plain solve's argument block
// there to the last bit), whose increment is the sum of the fine pair's, one rounded addition per component — for
// Heston on the correlated components.  monitor_every is even: the coarse monitor counts monitor_every/2 coarse steps,
// both legs see the same dates.  The layout is the antithetic one: column n_paths + i is trajectory i's coarse partner.
template <class M>
__global__ __launch_bounds__(256) void coupled_stats_kernel(const SimArgs<0> a, const SimArgs<0> ac, const double S0,
                                                            const uint32_t monitor_every, const int include_start,
                                                            double* __restrict__ stats) {
  using State = typename M::State;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, true);
  const uint32_t n_coarse = ac.n_steps;  // a.n_steps / 2
  State sf, sc;
  M::init(sf, a);
  M::init(sc, ac);
  Monitor<false> mf(monitor_every, include_start), mc(monitor_every >> 1, include_start);
  mf.start(S0, a.x0.v);
  mc.start(S0, ac.x0.v);
  const uint64_t key = a.seeds[i];
  for (uint32_t j = 0; j < n_coarse; ++j) {
    double d1a, d2a = 0.0, d1b, d2b = 0.0;
    if constexpr (M::NCOMP == 2) {
      euler_pair_increments(key, 2u * j, a, d1a, d2a);
      euler_pair_increments(key, 2u * j + 1u, a, d1b, d2b);
    } else {
      double z1, z2;
      euler_scalar_normals(key, j, z1, z2);  // one Philox block is one fine pair of steps
      d1a = a.sqrt_dt * z1;
      d1b = a.sqrt_dt * z2;
    }
    M::step(sf, a, d1a, d2a);
    mf.date(sf.x.v, sf.x.v);
    M::step(sf, a, d1b, d2b);
    mf.date(sf.x.v, sf.x.v);
    M::step(sc, ac, d1a + d1b, d2a + d2b);
    mc.date(sc.x.v, sc.x.v);
  }
  mf.store(stats, at, i, a.n_paths);
  mc.store(stats, at, a.n_paths + i, a.n_paths);
}

// path_payoff_kernel's sibling on coupled_stats_kernel's rows: the same block -> (chunk, payoff group) map, payoffs per
// load and lane order.  Per trajectory and payoff p_f on the fine rows, p_c on the coarse ones and Y = p_f − p_c, one
// rounded subtraction; Σ Y, Σ Y² into record group k and Σ p_f, Σ p_f² into group n_payoffs + k — the latter exactly as
// path_payoff_kernel accumulates a payoff that is not antithetic, so the fine sums are a plain solve's bit for bit.
__global__ __launch_bounds__(256) void level_payoff_kernel(const PathPayoffArgs b, const uint32_t n_payoffs) {
  const uint32_t per_xcd = (b.n_chunks + 7u) / 8u;
  const uint32_t xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
  const uint32_t grp = idx / per_xcd, chunk = (idx % per_xcd) * 8u + xcd;
  if (chunk >= b.n_chunks) return;
  const uint32_t k0 = grp * kPathKB;
  hh_path_payoff q[kPathKB];
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) q[g] = b.payoffs[min(k0 + g, n_payoffs - 1)];
  const PathStatsLayout at(b.n_paths, true);
  double acc_y[kPathKB][2], acc_f[kPathKB][2];
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) acc_y[g][0] = acc_y[g][1] = acc_f[g][0] = acc_f[g][1] = 0.0;
  const uint64_t i0 = (uint64_t)chunk * kBasketChunk;
  for (uint32_t j = threadIdx.x; j < (uint32_t)kBasketChunk; j += 256) {
    const uint64_t i = i0 + j;
    if (i >= b.n_paths) break;
    double tf[HH_PATH_STATS], tc[HH_PATH_STATS];
#pragma unroll
    for (int s = 0; s < HH_PATH_STATS; ++s) {
      tf[s] = b.stats[at.row(s) + i];
      tc[s] = b.stats[at.row(s) + b.n_paths + i];
    }
#pragma unroll
    for (int g = 0; g < kPathKB; ++g) {
      const bool live = k0 + g < n_payoffs;  // uniform over the workgroup
      const double pf = path_payoff_of(q[g], tf, b.n_mon);
      const double pc = path_payoff_of(q[g], tc, b.n_mon);
      if (b.values && live) {
        b.values[(size_t)(k0 + g) * at.n_total + i] = pf;
        b.values[(size_t)(k0 + g) * at.n_total + b.n_paths + i] = pc;
      }
      const double y = pf - pc;
      acc_y[g][0] += y;
      acc_y[g][1] = fma(y, y, acc_y[g][1]);
      acc_f[g][0] += pf;
      acc_f[g][1] = fma(pf, pf, acc_f[g][1]);
    }
  }
#pragma unroll
  for (int g = 0; g < kPathKB; ++g) {
    if (k0 + g >= n_payoffs) break;  // uniform over the workgroup
    if (g) __syncthreads();          // the reduction's LDS staging is reused
    block_reduce_store<2, 4, 0>(acc_y[g], b.records + ((size_t)(k0 + g) * b.n_chunks + chunk) * kRecStride);
    __syncthreads();
    block_reduce_store<2, 4, 0>(acc_f[g], b.records + ((size_t)(n_payoffs + k0 + g) * b.n_chunks + chunk) * kRecStride);
  }
}

}  // namespace

int launch_coupled_stats(const hh_model& m, const hh_config& c, const uint64_t* seeds_dev, uint32_t monitor_every,
                         bool include_start, double* stats, hipStream_t s) {
  const StatsLaunch fine(m, c, seeds_dev);
  hh_config cc = c;
  cc.n_steps = c.n_steps / 2;
  const StatsLaunch coarse(m, cc, seeds_dev);
  auto go = [&](auto model) {
    hipLaunchKernelGGL((coupled_stats_kernel<decltype(model)>), fine.grid, fine.block, 0, s, fine.a, coarse.a, m.S0,
                       monitor_every, (int)include_start, stats);
  };
  if (c.dynamics == HH_LOGNORMAL) go(GbmModel<0>{});
  else if (c.em_split) go(HestonModel<0, true>{});
  else go(HestonModel<0, false>{});
  return (int)hipGetLastError();
}

int launch_level_payoffs(const PathPayoffArgs& b, uint32_t n_payoffs, hipStream_t s) {
  const uint32_t n_groups = (n_payoffs + kPathKB - 1) / kPathKB;
  if ((uint64_t)((b.n_chunks + 7u) / 8u) * 8u * n_groups > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  const dim3 grid(((b.n_chunks + 7u) / 8u) * 8u * n_groups), block(256);
  hipLaunchKernelGGL(level_payoff_kernel, grid, block, 0, s, b, n_payoffs);
  return (int)hipGetLastError();
}

int launch_path_stats(const hh_model& m, const hh_config& c, const uint64_t* seeds_dev, uint32_t monitor_every,
                      bool include_start, bool bridge, double* stats, hipStream_t s, bool date_rows, bool state_rows) {
  const StatsLaunch l(m, c, seeds_dev);
  if (state_rows && c.dynamics != HH_HESTON) return (int)hipErrorInvalidValue;  // the entry point has refused it
  auto go = [&](auto model, auto anti, auto br) {
    hipLaunchKernelGGL((path_stats_kernel<decltype(model), decltype(anti)::value, decltype(br)::value>), l.grid, l.block, 0,
                       s, l.a, m.S0, monitor_every, (int)include_start, stats);
  };
  auto with_form = [&](auto model, auto anti) {
    constexpr bool kAnti = decltype(anti)::value;
    if constexpr (decltype(model)::NCOMP == 2) {
      if (state_rows) {
        hipLaunchKernelGGL((path_stats_kernel<decltype(model), kAnti, false, StateRows<kAnti>>), l.grid, l.block, 0, s, l.a,
                           m.S0, monitor_every, 1, stats);
        return;
      }
    }
    if (date_rows)
      hipLaunchKernelGGL((path_stats_kernel<decltype(model), kAnti, false, DateRows<kAnti>>), l.grid, l.block, 0, s, l.a, m.S0,
                         monitor_every, 1, stats);
    else if (bridge) go(model, anti, std::true_type{});
    else go(model, anti, std::false_type{});
  };
  auto with_anti = [&](auto model) {
    if (c.antithetic) with_form(model, std::true_type{});
    else with_form(model, std::false_type{});
  };
  if (c.dynamics == HH_LOGNORMAL) with_anti(GbmModel<0>{});
  else if (c.em_split) with_anti(HestonModel<0, true>{});
  else with_anti(HestonModel<0, false>{});
  return (int)hipGetLastError();
}

// The carried slots decide the instantiation: P = n_active (lognormal dynamics carry sigma alone: P <= 1).  P = 0 takes
// launch_path_stats' argument block.  No form spills, so the slots are never split over passes.
int launch_path_tangent(const hh_model& m, const hh_config& c, const uint64_t* seeds_dev, uint32_t monitor_every,
                        bool include_start, double* rows, hipStream_t s) {
  const StatsLaunch l(m, c, seeds_dev);
  DevicePtrs p{};
  p.seeds = seeds_dev;
  auto with_p = [&](auto p_c) {
    constexpr int P = decltype(p_c)::value;
    SimArgs<P> a;
    if constexpr (P == 0) a = l.a;
    else a = make_basis_args<P>(m, c, p);
    auto go = [&](auto model, auto anti) {
      hipLaunchKernelGGL((path_tangent_kernel<decltype(model), P, decltype(anti)::value>), l.grid, l.block, 0, s, a, m.S0,
                         monitor_every, (int)include_start, rows);
    };
    auto with_anti = [&](auto model) {
      if (c.antithetic) go(model, std::true_type{});
      else go(model, std::false_type{});
    };
    if constexpr (P <= 1) {
      if (c.dynamics == HH_LOGNORMAL) return with_anti(GbmModel<P>{});
    }
    if (c.em_split) with_anti(HestonModel<P, true>{});
    else with_anti(HestonModel<P, false>{});
  };
  switch (partial_map(m, c).n_active) {
    case 0: with_p(std::integral_constant<int, 0>{}); break;
    case 1: with_p(std::integral_constant<int, 1>{}); break;
    case 2: with_p(std::integral_constant<int, 2>{}); break;
    case 3: with_p(std::integral_constant<int, 3>{}); break;
    default: with_p(std::integral_constant<int, 4>{}); break;
  }
  return (int)hipGetLastError();
}

int launch_path_payoff_tangent(const PathTangentArgs& b, uint32_t n_payoffs, hipStream_t s) {
  const uint32_t n_groups = (n_payoffs + kPathKB - 1) / kPathKB;
  if ((uint64_t)((b.n_chunks + 7u) / 8u) * 8u * n_groups > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  const dim3 grid(((b.n_chunks + 7u) / 8u) * 8u * n_groups), block(256);
  hipLaunchKernelGGL(path_payoff_tangent_kernel, grid, block, 0, s, b, n_payoffs);
  return (int)hipGetLastError();
}

int launch_path_payoffs(const PathPayoffArgs& b, uint32_t n_payoffs, hipStream_t s) {
  const uint32_t n_groups = (n_payoffs + kPathKB - 1) / kPathKB;
  if ((uint64_t)((b.n_chunks + 7u) / 8u) * 8u * n_groups > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  const dim3 grid(((b.n_chunks + 7u) / 8u) * 8u * n_groups), block(256);
  hipLaunchKernelGGL(path_payoff_kernel, grid, block, 0, s, b, n_payoffs);
  return (int)hipGetLastError();
}

}  // namespace hh
