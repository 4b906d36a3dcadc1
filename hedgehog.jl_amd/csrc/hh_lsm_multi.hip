// Longstaff–Schwartz on SEVERAL state rows per date (include/hedgehog_mc.h, "American exercise on several state rows"):
// the backward induction of hh_lsm.hip with a regression basis in m variables — all monomials of total degree <= p of the
// standardised regressors, B = C(m + p, p) <= 45 of them, in the graded lexicographic order of hh_lsm_basis.h.  It reads a
// device grid rows[date][state][column] of m state rows per date and a by-value descriptor that says how a column's m
// states give (a) the exercise value and (b) the m regressors; it knows nothing else of where the rows come from.  The
// two descriptors are "log-states of assets" (hh_assets_path_rows): exercise value cp·(I − K) with I from index_of
// (hh_assets.h), regressors v_i = exp(x_i) — and "log spot and variance" (hh_mc_path_states, m = 2): exercise value
// cp·(exp(x_0) − K), regressors exp(x_0) and x_1, the variance as stored.  A descriptor is one more case in column_of and
// nowhere else.
//
// FORM: one launch per date, and that is the whole of it — there is no persistent / cooperative form of this induction
// (hh_lsm.hip has one for a single row; here B² running sums per workgroup would have to cross the chip per date).
// Ahead of the chain, for all regressed dates t = 1 .. n_dates−1 at once (they do not depend on decisions):
//   1. statistics  n, Σv_i, Σv_i² over the in-the-money columns (pay > 0)  -> μ_i, isd_i by rowstat_of's formulas
//      (n = 0: μ = 0, isd = 1; a variance not > 0: isd = 1), z_i = (v_i − μ_i)·isd_i
//   2. Gram sums   G_jk = Σ φ_j φ_k
// then the chain, date t = n_dates−1 down to 1: a one-wave solve of G c = b for row t (b_j = Σ φ_j·y, y = D^(τ−t)·val, left
// by the launch before), and a step launch that exercises at row t where pay > 0 and pay > φ·c and forms the moment sums
// of row t−1.  The price is hh_lsm.hip's final Σ, Σ² kernel on (τ, val).
//
// THE GRAM PASS is the hot one: 1035 + 45 running sums at B = 45, which no lane can hold.  It forms ΦᵀΦ with
// v_mfma_f64_16x16x4_f64: the basis is cut into NT = ⌈B/16⌉ <= 3 tiles of 16 functions, a wave keeps the NT(NT+1)/2 <= 6
// tile products of the upper block triangle as 16×16 accumulators of 8 registers each (48 in all), and one instruction
// adds four columns to a tile: lane l supplies φ_{16·ti + (l & 15)} as A and φ_{16·tj + (l & 15)} as B, both of column
// l >> 4 of the batch.  fp64 MFMA is no faster than the VALU on this chip; it is here for the registers.  A workgroup
// takes 512 columns at a time: lane-per-column, it forms pay, v_i, z_i and the start value (1 in the money, 0 not — so a
// column out of the money or beyond the ensemble adds exact zeros, branch-free) into LDS; then each wave walks ITS OWN 64
// columns in 16 batches of four.  24 – 52 KiB of LDS (the staged slice, 4 KiB per regressor, and the 16 KiB the waves' tiles
// are added through), 8 waves per workgroup, no scratch.  The moment sums use the same lane
// layout with the VALU: lane l adds φ_{16·t + (l & 15)}·y of column l >> 4 of every batch, three running sums.
//
// SUMMATION TREES — fixed, independent of the number of CUs and of scheduling; no floating-point atomics; the same inputs
// give the same bits on every run.  chunk = 512 lanes × Q columns (Q and the chunk count: lsm_q / lsm_nch of hh_layout.h,
// the one-variable induction's rule); column = chunk·512·Q + s·512 + lane, s = 0 .. Q−1 the chunk's SLICES.
//   statistics   a lane adds its Q columns in slice order; the wave adds its lanes by the butterfly (l, l^32), (l, l^16), …,
//                (l, l^1); the chunk adds its 8 waves in order; the date adds its chunks in order.
//   Gram sums    a wave adds the batches b = 0 .. 15 of its 64 columns of a slice in order (batch b = columns 4b .. 4b+3 of
//                the wave's 64; the matrix instruction adds the four products of a batch to the accumulator in the order
//                the hardware fixes), slice after slice; the chunk adds its 8 waves in order; the date its chunks in order.
//   moment sums  lane l adds column l >> 4 of the batches in order, slice after slice; the four lanes that share l & 15 are
//                added by (l, l^32), (l, l^16); then waves in order, chunks in order.
//   φ·c          c_0·φ_0 first, then fma(c_j, φ_j, ·) in basis order.
// THE SOLVE: LDLᵀ without pivoting on one wave, row j in lane j, the pivot row travelling by v_readlane — as
// solve_normal_equations_wave of hh_lsm.hip, its rule for a vanished pivot included: a pivot not above 1e-13 times the
// column's own diagonal entry G_cc is dropped, its coefficient 0.  B <= 45 fits the lanes.
#include <cmath>
#include <type_traits>

#include "hh_assets.h"
#include "hh_kernels.h"
#include "hh_layout.h"
#include "hh_lsm_basis.h"

namespace hh {
namespace {

constexpr int kWaves = kLsmWg / 64;
constexpr int kPad = kLsmBasisPad;          // 48: a padded basis, three tiles of 16
constexpr int kStatStride = 1 + 2 * HH_MAX_ASSETS;  // n, Σv_i (μ_i), Σv_i² (isd_i)
constexpr int kTilePairs = 6;               // the upper block triangle of 3 × 3 tiles
constexpr int kTileVals = 256;              // doubles of a 16 × 16 tile: [reg][lane], row (lane >> 4) + 4·reg, column lane & 15
static_assert(kPad == kLsmMultiPad && kStatStride == kLsmMultiStats && kTilePairs * kTileVals == kLsmMultiTileDoubles,
              "LsmMultiScratch (hh_layout.h) sizes these");

typedef double f64x4 __attribute__((ext_vector_type(4)));

// How a column's states give the exercise value and the regressors.  By value: wave-uniform.
struct StatesDesc {
  int32_t kind;        // enum hh_lsm_states_kind
  int32_t index_kind;  // HH_LSM_STATES_LOG_ASSETS: enum hh_index_kind
  double cp, strike;
  AssetArgs c;         // … and the weights of the index, where index_of reads them (c.w); nothing else is set
                       // (HH_LSM_STATES_LOG_SPOT_VARIANCE reads neither)
};

template <int M>
__device__ __forceinline__ void column_of(const StatesDesc& d, const double (&x)[M], double& pay, double (&v)[M]) {
  // HH_LSM_STATES_LOG_SPOT_VARIANCE (m = 2: the descriptor check admits no other): the spot and the variance as stored
  if constexpr (M == 2) {
    if (d.kind == HH_LSM_STATES_LOG_SPOT_VARIANCE) {  // uniform
      v[0] = exp(x[0]);
      v[1] = x[1];
      pay = d.cp * (v[0] - d.strike);
      return;
    }
  }
  // HH_LSM_STATES_LOG_ASSETS: the index as the statistics kernel forms it on these states
  double I, xi;
  switch (d.index_kind) {  // uniform
    case HH_INDEX_WEIGHTED_SUM: index_of<M, HH_INDEX_WEIGHTED_SUM>(d.c, x, I, xi); break;
    case HH_INDEX_GEOMETRIC: index_of<M, HH_INDEX_GEOMETRIC>(d.c, x, I, xi); break;
    case HH_INDEX_BEST_OF: index_of<M, HH_INDEX_BEST_OF>(d.c, x, I, xi); break;
    default: index_of<M, HH_INDEX_WORST_OF>(d.c, x, I, xi); break;
  }
  pay = d.cp * (I - d.strike);
#pragma unroll
  for (int i = 0; i < M; ++i) v[i] = exp(x[i]);
}

struct MultiArgs {
  const double* rows;  // [n_dates + 1][m][ntot]
  uint64_t ntot;
  uint32_t n_dates, n_chunks;
  int32_t q, B, n_tiles, p;  // p: the degree
  StatesDesc d;
  int32_t* tau;
  double* val;
  double* rec_stats;       // [date][chunk][kStatStride]
  double* rowstat;         // [date][kStatStride]: n, μ_i at 1 + i, isd_i at 1 + HH_MAX_ASSETS + i
  double* rec_gram;        // [date of the block][chunk][kTilePairs][kTileVals]
  double* G;               // [date][kPad][kPad]
  double* recB;            // [date][chunk][kPad]
  double* coef;            // [date][kPad], zeros where no fit ran
  int32_t* have_fit;       // [date]
  const double* disc_pow;  // [k] = D^k
  double* counters;        // rows regressed, rows skipped
  uint32_t expo[kPad];     // the basis (hh_lsm_basis.h), padded with kLsmNoBasis
};

// (l, l^OFF) of a wave
template <int OFF>
__device__ __forceinline__ double xor_add(double x) {
  return x + __shfl_xor(x, OFF, 64);
}
__device__ __forceinline__ double wave_sum(double x) {
  x = xor_add<32>(x);
  x = xor_add<16>(x);
  x = xor_add<8>(x);
  x = xor_add<4>(x);
  x = xor_add<2>(x);
  return xor_add<1>(x);
}

// rec[0] + rec[stride] + … over n records, added IN ORDER; the loads of 16 records are issued together, so a date costs
// n/16 trips to memory instead of n (the sum, and so every bit of it, is the serial one)
__device__ __forceinline__ double ordered_sum(const double* __restrict__ rec, uint32_t n, size_t stride) {
  double t = 0.0;
  uint32_t ch = 0;
  for (; ch + 16 <= n; ch += 16) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = rec[(size_t)(ch + k) * stride];
#pragma unroll
    for (int k = 0; k < 16; ++k) t += v[k];
  }
  for (; ch < n; ++ch) t += rec[(size_t)ch * stride];
  return t;
}

// the m states of column `col` of date `row` (col < ntot)
template <int M>
__device__ __forceinline__ void load_states(const MultiArgs& a, uint32_t row, uint64_t col, double (&x)[M]) {
  const double* p = a.rows + ((size_t)row * M) * a.ntot + col;
#pragma unroll
  for (int i = 0; i < M; ++i) x[i] = p[(size_t)i * a.ntot];
}

// z_i of a column from the date's statistics; returns the start value of its φ (1 in the money, 0 not)
template <int M>
__device__ __forceinline__ double standardise(const double* __restrict__ rs, const double (&v)[M], double pay, bool live,
                                              double (&z)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) z[i] = (v[i] - rs[1 + i]) * rs[1 + HH_MAX_ASSETS + i];
  return live && pay > 0.0 ? 1.0 : 0.0;
}

// ---- ahead of the chain: statistics and Gram sums of every regressed date -------------------------------------------

template <int M>
__global__ __launch_bounds__(kLsmWg) void multi_stats_kernel(const MultiArgs a) {
  constexpr int NV = 1 + 2 * M;
  __shared__ double part[kWaves][NV];
  const uint32_t chunk = blockIdx.x, row = blockIdx.y + 1;
  double n = 0.0, sv[M], svv[M];
#pragma unroll
  for (int i = 0; i < M; ++i) sv[i] = svv[i] = 0.0;
  for (int s = 0; s < a.q; ++s) {
    const uint64_t p = (uint64_t)chunk * ((uint64_t)kLsmWg * a.q) + (uint64_t)s * kLsmWg + threadIdx.x;
    const bool live = p < a.ntot;
    double x[M], v[M], pay;
    load_states<M>(a, row, live ? p : a.ntot - 1, x);
    column_of<M>(a.d, x, pay, v);
    const bool itm = live && pay > 0.0;
    n += itm ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const double vm = itm ? v[i] : 0.0;
      sv[i] += vm;
      svv[i] = fma(vm, vm, svv[i]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  n = wave_sum(n);
  if (lane == 0) part[wave][0] = n;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const double s1 = wave_sum(sv[i]), s2 = wave_sum(svv[i]);
    if (lane == 0) {
      part[wave][1 + i] = s1;
      part[wave][1 + M + i] = s2;
    }
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += part[w][threadIdx.x];
    const int slot = threadIdx.x == 0 ? 0 : threadIdx.x <= M ? (int)threadIdx.x : 1 + HH_MAX_ASSETS + ((int)threadIdx.x - 1 - M);
    a.rec_stats[((size_t)row * a.n_chunks + chunk) * kStatStride + slot] = t;
  }
}

// the date's chunks in order, then rowstat_of's formulas per regressor (grid = regressed dates, one wave)
__global__ __launch_bounds__(64) void multi_rowstat_kernel(const MultiArgs a, int m) {
  __shared__ double tot[kStatStride];
  const uint32_t row = blockIdx.x + 1;
  const int k = threadIdx.x;
  if (k < kStatStride) {
    const bool used = k == 0 || (k >= 1 && k < 1 + m) || (k >= 1 + HH_MAX_ASSETS && k < 1 + HH_MAX_ASSETS + m);
    tot[k] = used ? ordered_sum(a.rec_stats + (size_t)row * a.n_chunks * kStatStride + k, a.n_chunks, kStatStride) : 0.0;
  }
  __syncthreads();
  double* rs = a.rowstat + (size_t)row * kStatStride;
  const double n = tot[0];
  if (k == 0) rs[0] = n;
  if (k < HH_MAX_ASSETS) {
    double mu = 0.0, isd = 1.0;
    if (k < m && n > 0.0) {
      mu = tot[1 + k] / n;
      const double var = tot[1 + HH_MAX_ASSETS + k] / n - mu * mu;
      isd = var > 0.0 ? 1.0 / sqrt(var) : 1.0;
    }
    rs[1 + k] = mu;
    rs[1 + HH_MAX_ASSETS + k] = isd;
  }
}

// A slice of 512 columns of date `row` into LDS, lane per column: the start value and the z_i.
template <int M>
__device__ __forceinline__ void stage_slice(const MultiArgs& a, uint32_t row, const double* __restrict__ rs, uint64_t p,
                                            double* __restrict__ sbuf, double* __restrict__ zbuf) {
  const bool live = p < a.ntot;
  double x[M], v[M], z[M], pay;
  load_states<M>(a, row, live ? p : a.ntot - 1, x);
  column_of<M>(a.d, x, pay, v);
  sbuf[threadIdx.x] = standardise<M>(rs, v, pay, live, z);
#pragma unroll
  for (int i = 0; i < M; ++i) zbuf[i * kLsmWg + threadIdx.x] = z[i];
}

// the pair index of tiles (ti <= tj) in the upper block triangle of 3 × 3
__host__ __device__ constexpr int tile_pair(int ti, int tj) { return ti == 0 ? tj : ti == 1 ? 2 + tj : 5; }

template <int M, int NT>
__global__ __launch_bounds__(kLsmWg) void multi_gram_kernel(const MultiArgs a, uint32_t row0) {
  constexpr int P = lsm_max_degree(M);
  __shared__ double sbuf[kLsmWg], zbuf[M * kLsmWg], rs[kStatStride];
  __shared__ double red[kWaves * kTileVals];
  const uint32_t chunk = blockIdx.x, row = row0 + blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kStatStride) rs[threadIdx.x] = a.rowstat[(size_t)row * kStatStride + threadIdx.x];
  uint32_t e[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) e[t] = a.expo[16 * t + (lane & 15)];
  f64x4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int k = 0; k < NT * (NT + 1) / 2; ++k) acc[k] = f64x4{0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  for (int s = 0; s < a.q; ++s) {
    const uint64_t p = (uint64_t)chunk * ((uint64_t)kLsmWg * a.q) + (uint64_t)s * kLsmWg + threadIdx.x;
    stage_slice<M>(a, row, rs, p, sbuf, zbuf);
    __syncthreads();
#pragma unroll 2
    for (int b = 0; b < 16; ++b) {
      const int col = wave * 64 + 4 * b + (lane >> 4);
      double z[M];
#pragma unroll
      for (int i = 0; i < M; ++i) z[i] = zbuf[i * kLsmWg + col];
      const double start = sbuf[col];
      double f[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) f[t] = lsm_phi<M, P>(start, z, e[t], a.p);
      int k = 0;
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = ti; tj < NT; ++tj, ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[ti], f[tj], acc[k], 0, 0, 0);
    }
    __syncthreads();
  }
  // the chunk's 8 waves in order, tile by tile
  double* rec = a.rec_gram + ((size_t)blockIdx.y * a.n_chunks + chunk) * (kTilePairs * kTileVals);
  int k = 0;
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int tj = ti; tj < NT; ++tj, ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * kTileVals + r * 64 + lane] = acc[k][r];
      __syncthreads();
      if (threadIdx.x < kTileVals) {
        double t = red[threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += red[w * kTileVals + threadIdx.x];
        rec[tile_pair(ti, tj) * kTileVals + threadIdx.x] = t;
      }
      __syncthreads();
    }
}

// G of the block's dates: the chunks in order, each entry to its place (grid = (dates of the block, tile pairs))
__global__ __launch_bounds__(kTileVals) void multi_gram_sum_kernel(const MultiArgs a, uint32_t row0) {
  const uint32_t row = row0 + blockIdx.x;
  const int pair = blockIdx.y;
  const int ti = pair < 3 ? 0 : pair < 5 ? 1 : 2, tj = pair < 3 ? pair : pair < 5 ? pair - 2 : 2;
  if (tj >= a.n_tiles) return;
  const int lane = threadIdx.x & 63, reg = threadIdx.x >> 6;
  const double* rec = a.rec_gram + (size_t)blockIdx.x * a.n_chunks * (kTilePairs * kTileVals) + pair * kTileVals + threadIdx.x;
  const double t = ordered_sum(rec, a.n_chunks, kTilePairs * kTileVals);
  const int j = 16 * ti + (lane >> 4) + 4 * reg, k = 16 * tj + (lane & 15);
  double* G = a.G + (size_t)row * kPad * kPad;
  G[j * kPad + k] = t;
  if (ti != tj) G[k * kPad + j] = t;
}

// ---- the chain ------------------------------------------------------------------------------------------------------

// 1/x to <= 1 ulp: the hardware reciprocal and two Newton steps, as hh_lsm.hip's
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// G c = b of date t on one wave: b from the chunk records in order, then the LDLᵀ of the head comment.  N: the padded
// order the loops are unrolled to (16, 32 or 48); steps at and beyond B are skipped by uniform branches.
template <int N>
__global__ __launch_bounds__(64) void multi_solve_kernel(const MultiArgs a, uint32_t t) {
  constexpr int kStage = 64;  // chunk records staged at a time: the chain waits for n_chunks/64 trips to memory per date
  __shared__ double stage[kStage * kPad];
  const int lane = threadIdx.x, B = a.B;
  const double n_itm = a.rowstat[(size_t)t * kStatStride];
  const bool fit = n_itm > 0.0;  // isempty(in_the_money) && continue
  double cf = 0.0;
  if (fit) {
    const bool mine = lane < B;
    double rhs = 0.0;
    const double* rec = a.recB + (size_t)t * a.n_chunks * kPad;  // [chunk][kPad], contiguous: the wave reads whole lines
    for (uint32_t base = 0; base < a.n_chunks; base += kStage) {
      const uint32_t cnt = a.n_chunks - base < (uint32_t)kStage ? a.n_chunks - base : (uint32_t)kStage;
#pragma unroll 8
      for (uint32_t k = lane; k < cnt * kPad; k += 64) stage[k] = rec[(size_t)base * kPad + k];
      __syncthreads();
      if (mine)
        for (uint32_t ch = 0; ch < cnt; ++ch) rhs += stage[ch * kPad + lane];  // the chunks in order
      __syncthreads();
    }
    const double* Grow = a.G + ((size_t)t * kPad + (mine ? lane : 0)) * kPad;
    double r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = mine && k < B ? Grow[k] : 0.0;
    const double diag0 = mine ? Grow[lane] : 0.0;
    double myinv = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      if (c < B) {
        const double piv = readlane_f64(r[c], c);
        const bool dead = !(piv > 1e-13 * readlane_f64(diag0, c));
        const double inv = dead ? 0.0 : rcp_nr(piv);
        if (lane == c) myinv = inv;
        if (!dead) {
          const bool below = lane > c;
          const double f = below ? r[c] * inv : 0.0;
#pragma unroll
          for (int k = c; k < N; ++k) {
            if (k < B) {
              const double pk = readlane_f64(r[k], c);
              r[k] = below ? fma(-f, pk, r[k]) : r[k];
            }
          }
          const double pb = readlane_f64(rhs, c);
          rhs = below ? fma(-f, pb, rhs) : rhs;
        }
      }
    }
    // back-substitution by columns: lane c holds the final row c; its unknown is broadcast and leaves the rows above
#pragma unroll
    for (int c = N - 1; c >= 0; --c) {
      if (c < B) {
        const double xc = readlane_f64(rhs * myinv, c);  // 0 for a dropped column
        if (lane == c) cf = xc;
        rhs = lane < c ? fma(-r[c], xc, rhs) : rhs;
      }
    }
  }
  if (lane < kPad) a.coef[(size_t)t * kPad + lane] = lane < B ? cf : 0.0;
  if (lane == 0) {
    a.have_fit[t] = fit ? 1 : 0;
    a.counters[fit ? 0 : 1] += 1.0;
  }
}

// this chunk's Σ φ_j·y of date `row` from the lanes' three running sums into recB[row][chunk]
__device__ __forceinline__ void store_moments(const MultiArgs& a, uint32_t row, double (&m)[3], double* part /*[kWaves][kPad]*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    double s = xor_add<32>(m[t]);
    s = xor_add<16>(s);
    if (lane < 16) part[wave * kPad + 16 * t + lane] = s;
  }
  __syncthreads();
  if (threadIdx.x < kPad) {
    double t = part[threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += part[w * kPad + threadIdx.x];
    a.recB[((size_t)row * a.n_chunks + blockIdx.x) * kPad + threadIdx.x] = t;
  }
}

// the wave's 64 staged columns (start value, z_i, y in LDS) into the lanes' running sums: Σ φ·y in the lane layout
template <int M>
__device__ __forceinline__ void add_moments(const MultiArgs& a, const uint32_t (&e)[3], const double* __restrict__ sbuf,
                                            const double* __restrict__ zbuf, const double* __restrict__ ybuf, double (&m)[3]) {
  constexpr int P = lsm_max_degree(M);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 2
  for (int b = 0; b < 16; ++b) {
    const int col = wave * 64 + 4 * b + (lane >> 4);
    double z[M];
#pragma unroll
    for (int i = 0; i < M; ++i) z[i] = zbuf[i * kLsmWg + col];
    const double start = sbuf[col], y = ybuf[col];
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (t < a.n_tiles) m[t] += lsm_phi<M, P>(start, z, e[t], a.p) * y;  // a tile beyond the basis holds zeros: skipped
  }
}

// One backward step at date t (t == n_dates: the start — τ = n_dates, val = the payoff at expiry): the decisions of row
// t, then this chunk's moment sums of row t − 1 with the stopping state as of now.
template <int M>
__global__ __launch_bounds__(kLsmWg) void multi_step_kernel(const MultiArgs a, uint32_t t) {
  constexpr int P = lsm_max_degree(M);
  __shared__ double sbuf[kLsmWg], ybuf[kLsmWg], zbuf[M * kLsmWg], part[kWaves * kPad];
  __shared__ double rs[kStatStride], rsn[kStatStride], coef[kPad];
  __shared__ uint32_t expo[kPad];
  const bool first = t == a.n_dates, more = t >= 2;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < kPad) {
    expo[threadIdx.x] = a.expo[threadIdx.x];
    coef[threadIdx.x] = first ? 0.0 : a.coef[(size_t)t * kPad + threadIdx.x];
  }
  if (threadIdx.x < kStatStride) {
    rs[threadIdx.x] = first ? 0.0 : a.rowstat[(size_t)t * kStatStride + threadIdx.x];
    rsn[threadIdx.x] = more ? a.rowstat[(size_t)(t - 1) * kStatStride + threadIdx.x] : 0.0;
  }
  const bool fit = !first && a.have_fit[t] != 0;
  uint32_t e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = a.expo[16 * k + (lane & 15)];
  double m[3] = {0.0, 0.0, 0.0};
  __syncthreads();
  for (int s = 0; s < a.q; ++s) {
    const uint64_t p = (uint64_t)blockIdx.x * ((uint64_t)kLsmWg * a.q) + (uint64_t)s * kLsmWg + threadIdx.x;
    const bool live = p < a.ntot;
    const uint64_t pc = live ? p : a.ntot - 1;
    double x[M], v[M], z[M], pay;
    load_states<M>(a, t, pc, x);
    column_of<M>(a.d, x, pay, v);
    int tau;
    double val;
    if (first) {
      tau = (int)t;
      val = pay > 0.0 ? pay : 0.0;
      if (live) {
        a.tau[p] = tau;
        a.val[p] = val;
      }
    } else {
      tau = a.tau[pc];
      val = a.val[pc];
      if (fit) {  // uniform
        standardise<M>(rs, v, pay, live, z);
        double cont = coef[0] * lsm_phi<M, P>(1.0, z, expo[0], a.p);
        for (int j = 1; j < a.B; ++j) cont = fma(coef[j], lsm_phi<M, P>(1.0, z, expo[j], a.p), cont);
        if (live && pay > 0.0 && pay > cont) {
          tau = (int)t;
          val = pay;
          a.tau[p] = tau;
          a.val[p] = val;
        }
      }
    }
    if (more) {  // uniform
      load_states<M>(a, t - 1, pc, x);
      column_of<M>(a.d, x, pay, v);
      sbuf[threadIdx.x] = standardise<M>(rsn, v, pay, live, z);
      ybuf[threadIdx.x] = live && pay > 0.0 ? a.disc_pow[tau - (int)(t - 1)] * val : 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) zbuf[i * kLsmWg + threadIdx.x] = z[i];
      __syncthreads();
      add_moments<M>(a, e, sbuf, zbuf, ybuf, m);
      __syncthreads();
    }
  }
  if (more) store_moments(a, t - 1, m, part);
}

// D^k for every k the induction can ask for
__global__ __launch_bounds__(256) void multi_disc_kernel(double ln_disc, uint32_t n, double* out) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k <= n) out[k] = exp(ln_disc * (double)k);
}

// ---- a policy run forward (include/hedgehog_mc.h, "Dual bounds for American exercise") -----------------------------------

struct PolicyArgs {
  const double* rows;    // [n_dates + 1][m][ntot]
  const double* policy;  // [n_dates + 1][2m + B]: μ_i, isd_i, coef_j of every date
  uint64_t ntot;
  uint32_t n_dates;
  int32_t B, p;          // p: the degree
  StatesDesc d;
  int32_t* tau;
  double* val;
  uint32_t expo[kPad];
};

// One lane per column, dates 1 .. n_dates in order: the first date the policy exercises, else expiry.  The fitted value is
// multi_step_kernel's, statement for statement — z_i from (μ_i, isd_i), c_0·φ_0, then fma in basis order, φ by lsm_phi — so
// on the rows a policy was fitted on a column stops where the induction stopped it.  Memory-bound: a date's m rows are
// read once, a wave's 64 columns one line each; the date's policy sits at a wave-uniform address (scalar loads).  A lane
// that has stopped leaves; no sum is formed here (launch_lsm_final has the induction's).
template <int M>
__global__ __launch_bounds__(256) void policy_value_kernel(const PolicyArgs a) {
  constexpr int P = lsm_max_degree(M);
  const uint64_t col = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.ntot) return;
  const int stride = 2 * M + a.B;
  int tau = (int)a.n_dates;
  double val = 0.0;
  double xn[M];  // the next date's states, asked for one date ahead: the loads travel while this date is evaluated
#pragma unroll
  for (int i = 0; i < M; ++i) xn[i] = a.rows[((size_t)M + i) * a.ntot + col];
  for (uint32_t t = 1; t <= a.n_dates; ++t) {
    double x[M], v[M], z[M], pay;
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = xn[i];
    if (t < a.n_dates) {  // uniform
      const double* r = a.rows + ((size_t)(t + 1) * M) * a.ntot + col;
#pragma unroll
      for (int i = 0; i < M; ++i) xn[i] = r[(size_t)i * a.ntot];
    }
    column_of<M>(a.d, x, pay, v);
    if (t == a.n_dates) {  // uniform
      val = pay > 0.0 ? pay : 0.0;
      break;
    }
    const double* __restrict__ pol = a.policy + (size_t)t * stride;
#pragma unroll
    for (int i = 0; i < M; ++i) z[i] = (v[i] - pol[i]) * pol[M + i];
    double cont = pol[2 * M] * lsm_phi<M, P>(1.0, z, a.expo[0], a.p);
    for (int j = 1; j < a.B; ++j) cont = fma(pol[2 * M + j], lsm_phi<M, P>(1.0, z, a.expo[j], a.p), cont);
    if (pay > 0.0 && pay > cont) {
      tau = (int)t;
      val = pay;
      break;
    }
  }
  a.tau[col] = tau;
  a.val[col] = val;
}

template <class F>
inline void with_m(int m, F&& f) {
  switch (m) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

}  // namespace

// The whole induction on `rows` ([n_dates + 1][m][ntot], device).  tau / val: ntot entries; scratch: LsmMultiScratch::total
// doubles; records: lsm_chunks(ntot) × kRecStride, left holding the Σ, Σ² of the discounted stopped values.  The entry
// points have checked every argument (1 <= m <= HH_MAX_ASSETS, lsm_basis_count(m, degree) > 0).
int launch_lsm_multi(const hh_lsm_states& desc, const double* rows, uint64_t ntot, uint32_t n_dates, int degree,
                     double date_discount, int32_t* tau, double* val, double* scratch, double* records, hipStream_t s) {
  const int m = (int)desc.n_states;
  MultiArgs a{};
  a.B = lsm_basis_fill(m, degree, a.expo);
  if (a.B == 0) return (int)hipErrorInvalidValue;
  const LsmMultiScratch at(ntot, n_dates);
  a.rows = rows; a.ntot = ntot; a.n_dates = n_dates; a.n_chunks = at.nch; a.q = at.q;
  a.n_tiles = (a.B + 15) / 16;
  a.p = degree;
  a.d.kind = desc.kind; a.d.index_kind = desc.index_kind; a.d.cp = desc.cp; a.d.strike = desc.strike;
  for (int i = 0; i < m; ++i) a.d.c.w[i] = desc.weights[i];
  a.tau = tau; a.val = val;
  a.rec_stats = scratch + at.rec_stats; a.rowstat = scratch + at.rowstat; a.rec_gram = scratch + at.rec_gram;
  a.G = scratch + at.G; a.recB = scratch + at.recB; a.coef = scratch + at.coef;
  a.have_fit = reinterpret_cast<int32_t*>(scratch + at.have_fit);
  a.disc_pow = scratch + at.disc_pow; a.counters = scratch + at.counters;
  const double ln_disc = log(date_discount);
  // coefficients, fit flags, the discount table's place and the counters start from zero: [coef, total)
  hipError_t e = hipMemsetAsync(scratch + at.coef, 0, (at.total - at.coef) * sizeof(double), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(multi_disc_kernel, dim3((at.rows + 255) / 256), dim3(256), 0, s, ln_disc, n_dates, scratch + at.disc_pow);
  const uint32_t n_fit = n_dates - 1;  // dates 1 .. n_dates − 1 are regressed
  with_m(m, [&](auto mc) {
    constexpr int M = decltype(mc)::value;
    if (n_fit) {
      hipLaunchKernelGGL(multi_stats_kernel<M>, dim3(at.nch, n_fit), dim3(kLsmWg), 0, s, a);
      hipLaunchKernelGGL(multi_rowstat_kernel, dim3(n_fit), dim3(64), 0, s, a, m);
      for (uint32_t row0 = 1; row0 <= n_fit; row0 += kLsmMultiRowBlock) {
        const uint32_t nb = n_fit - row0 + 1 < (uint32_t)kLsmMultiRowBlock ? n_fit - row0 + 1 : (uint32_t)kLsmMultiRowBlock;
        const dim3 g(at.nch, nb), b(kLsmWg);
        if (a.n_tiles == 1) hipLaunchKernelGGL((multi_gram_kernel<M, 1>), g, b, 0, s, a, row0);
        else if (a.n_tiles == 2) hipLaunchKernelGGL((multi_gram_kernel<M, 2>), g, b, 0, s, a, row0);
        else hipLaunchKernelGGL((multi_gram_kernel<M, 3>), g, b, 0, s, a, row0);
        hipLaunchKernelGGL(multi_gram_sum_kernel, dim3(nb, kTilePairs), dim3(kTileVals), 0, s, a, row0);
      }
    }
    hipLaunchKernelGGL(multi_step_kernel<M>, dim3(at.nch), dim3(kLsmWg), 0, s, a, n_dates);
    for (uint32_t t = n_dates - 1; t >= 1; --t) {
      if (a.n_tiles == 1) hipLaunchKernelGGL(multi_solve_kernel<16>, dim3(1), dim3(64), 0, s, a, t);
      else if (a.n_tiles == 2) hipLaunchKernelGGL(multi_solve_kernel<32>, dim3(1), dim3(64), 0, s, a, t);
      else hipLaunchKernelGGL(multi_solve_kernel<48>, dim3(1), dim3(64), 0, s, a, t);
      hipLaunchKernelGGL(multi_step_kernel<M>, dim3(at.nch), dim3(kLsmWg), 0, s, a, t);
    }
  });
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return launch_lsm_final(tau, val, ntot, ln_disc, records, s);
}

// A policy ([n_dates + 1][2m + B], device) run forward on `rows`: tau / val of every column, then the induction's final
// Σ, Σ² kernel into records (lsm_chunks(ntot) × kRecStride).  The entry points have checked every argument.
int launch_policy_value(const hh_lsm_states& desc, const double* rows, uint64_t ntot, uint32_t n_dates, int degree,
                        double date_discount, const double* policy, int32_t* tau, double* val, double* records,
                        hipStream_t s) {
  const int m = (int)desc.n_states;
  PolicyArgs a{};
  a.B = lsm_basis_fill(m, degree, a.expo);
  if (a.B == 0) return (int)hipErrorInvalidValue;
  a.rows = rows; a.policy = policy; a.ntot = ntot; a.n_dates = n_dates; a.p = degree;
  a.d.kind = desc.kind; a.d.index_kind = desc.index_kind; a.d.cp = desc.cp; a.d.strike = desc.strike;
  for (int i = 0; i < m; ++i) a.d.c.w[i] = desc.weights[i];
  a.tau = tau; a.val = val;
  with_m(m, [&](auto mc) {
    constexpr int M = decltype(mc)::value;
    hipLaunchKernelGGL(policy_value_kernel<M>, dim3((unsigned)((ntot + 255) / 256)), dim3(256), 0, s, a);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return launch_lsm_final(tau, val, ntot, log(date_discount), records, s);
}

}  // namespace hh
