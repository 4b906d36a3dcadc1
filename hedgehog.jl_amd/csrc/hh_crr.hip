// Cox–Ross–Rubinstein binomial trees on the device: solve(prob, ::CoxRossRubinsteinMethod) for a European or
// American VanillaOption on BlackScholesInputs (reference: src/pricing_methods/cox_ross_rubinstein.jl:99-141),
// a basket of trees in one launch (hh_crr_solve, include/hedgehog_mc.h).  DESIGN §5.8.
//
// A tree is a serial chain of N backward steps over a row that shrinks by one node per step.  One workgroup
// prices one tree; node j of the row lives in register c = j / WG of thread j % WG ("interleaved"), so at step i
// only registers c <= (i + 1) / WG hold live nodes and that bound is uniform: dead registers are skipped with
// scalar branches, and the work tracks N²/2.  The neighbour v[j + 1] is lane l + 1 of the same register (a
// rotate in the wave, ds_bpermute); lane 63 takes lane 0 of the NEXT wave (an LDS slot written before a barrier,
// double-buffered: one barrier per step) or, in the last wave, register c + 1 of thread 0 (a v_readlane when
// the workgroup is one wave).  Two forms, chosen by N alone so that a basket's prices equal single solves:
//   form A  N <= HH_CRR_FORM_A_MAX_STEPS: one wave per tree, C in {1, 2, 4, 8, 16, 32} registers per lane;
//   form B  larger N: 1024 threads per tree, C in {4, 8, 16, 33}.
//
// Arithmetic (fp64, no FMA contraction — the build passes -ffp-contract=off and this file says so again):
//   continuation   disc · ((p · v[j+1]) + (q · v[j])),  q = 1 − p, each operation rounded on its own — the
//                  reference's `p * value[2:end] + (1 - p) * value[1:end-1]`, then `discount_factor * continuation`;
//   exercise       max(cp · (S − K), 0), then max(continuation, exercise)  (American, every step i = N−1 … 0);
//   S              F · w_k (forward nodes, the leaves of both underlyings) or sf_i · (F · w_k) (Spot American);
//   node factors   w_k = u^k for k = 2j − i, by this fixed IEEE sequence (a device pow is not reproducible):
//                    pw(e) = u^e by left-to-right square-and-multiply: x = u, then for each bit of e below the
//                            leading one: x = x·x, and x = x·u when the bit is set; pw(0) = 1;
//                    m = |k|,  L = pw(m mod 256),  H = pw(256·⌊m / 256⌋),
//                    k >= 0:  w_k = H · L
//                    k <  0:  w_k = (1 / H) · (1 / L)
//                  (H = 1 when m < 256 and L = 1 when 256 | m, so those products are exact).  The 2·256 + 2·129
//                  factors sit in LDS, the L halves split by the parity of m: the lanes of one register read
//                  consecutive doubles.
// Every loop is bounded by N (or by the 770 table entries), whatever the scalars hold: NaN or infinite inputs
// give NaN or infinite prices, never a longer run.
#include <cmath>
#include <cstring>
#include <vector>

#include "hh_ctx.h"

#pragma clang fp contract(off)

namespace hh {

namespace {

constexpr int kLow = 256;                          // L: u^r, r < 256
constexpr int kHighN = HH_CRR_MAX_STEPS / kLow + 1;  // H: u^(256 m), m <= 128
constexpr int kTabLN = kLow;                       // offsets in the LDS table
constexpr int kTabHP = 2 * kLow;
constexpr int kTabHN = 2 * kLow + kHighN;
constexpr int kTab = 2 * kLow + 2 * kHighN;

__device__ __forceinline__ double pw(double u, int e) {
  if (e == 0) return 1.0;
  double x = u;
  const int top = 31 - __clz(e);
  for (int b = top - 1; b >= 0; --b) {  // at most 15 rounds (e <= 32768)
    x = x * x;
    if ((e >> b) & 1) x = x * u;
  }
  return x;
}

// entry e of the table: [0, 256) u^r and [256, 512) u^-r, each half ordered as r even then r odd
// (r = 2·(e mod 128) + (e mod 256) / 128); [512, 641) u^(256 m), [641, 770) u^(-256 m)
__device__ __forceinline__ double table_entry(double u, int e) {
  if (e < 2 * kLow) {
    const int s = e & (kLow - 1);
    const int r = 2 * (s & (kLow / 2 - 1)) + (s >> 7);
    const double x = pw(u, r);
    return e < kLow ? x : 1.0 / x;
  }
  const int m = e < kTabHN ? e - kTabHP : e - kTabHN;
  const double x = pw(u, kLow * m);
  return e < kTabHN ? x : 1.0 / x;
}

// w_k from the table; |k| is clamped to N (the nodes past the live row compute values nobody reads)
__device__ __forceinline__ double node_factor(const double* tab, int k, int N) {
  const bool neg = k < 0;
  int m = neg ? -k : k;
  m = m < N ? m : N;
  const int s = m & (kLow - 1);
  const int li = (neg ? kTabLN : 0) + ((s & 1) << 7) + (s >> 1);
  const int hi = (neg ? kTabHN : kTabHP) + (m >> 8);
  return tab[hi] * tab[li];
}

__device__ __forceinline__ double payoff(double cp, double S, double K) { return fmax(cp * (S - K), 0.0); }

__device__ __forceinline__ double read_lane0(double x) {
  const unsigned long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)(unsigned)b, 0);
  const int hi = __builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 0);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// NW waves per tree, C registers per lane: N + 1 <= 64·NW·C
template <int NW, int C>
__global__ __launch_bounds__(64 * NW) void crr_kernel(const CrrTree* __restrict__ trees,
                                                      const double* __restrict__ spot_factors, int N,
                                                      double* __restrict__ out) {
  constexpr int WG = 64 * NW;
  __shared__ double tab[kTab];
  __shared__ double edge[NW > 1 ? 2 : 1][C + 1][NW];  // lane 0's registers, per wave (form B)
  const CrrTree tr = trees[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int e = t; e < kTab; e += WG) tab[e] = table_entry(tr.u, e);
  __syncthreads();
  const double F = tr.F, K = tr.K, cp = tr.cp, p = tr.p, q = tr.q, disc = tr.disc;
  const bool american = tr.style != HH_CRR_EUROPEAN;
  const double* sf = tr.style == HH_CRR_AMERICAN_SPOT ? spot_factors + (size_t)tr.row * N : nullptr;

  double v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {  // leaves: payoff(F·w_k), k = 2j − N, on the forward for both underlyings
    const int j = c * WG + t;
    v[c] = j <= N ? payoff(cp, F * node_factor(tab, 2 * j - N, N), K) : 0.0;
  }
  const int src = (lane + 1) & 63;
  int buf = 0;
  for (int i = N - 1; i >= 0; --i) {
    const int live = (i + 1) / WG;  // registers holding nodes <= i + 1 (read)
    const int upd = i / WG;         // registers holding nodes <= i (written)
    if constexpr (NW > 1) {
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (c <= live) edge[buf][c][w] = v[c];
      }
      __syncthreads();
    }
    const double s_i = sf ? sf[i] : 1.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c <= upd) {  // a scalar branch: upd is uniform
        double nb = __shfl(v[c], src, 64);
        double nb63;
        if constexpr (NW == 1) {
          nb63 = (c + 1 < C) ? read_lane0(v[c + 1 < C ? c + 1 : c]) : 0.0;
        } else {
          nb63 = (w + 1 < NW) ? edge[buf][c][w + 1 < NW ? w + 1 : 0] : (c + 1 < C ? edge[buf][c + 1][0] : 0.0);
        }
        if (lane == 63) nb = nb63;
        const double pa = p * nb;
        const double qb = q * v[c];
        const double sum = pa + qb;
        double val = disc * sum;
        if (american) {
          const int j = c * WG + t;
          const double S = F * node_factor(tab, 2 * j - i, N);
          const double ex = payoff(cp, sf ? s_i * S : S, K);
          val = fmax(val, ex);
        }
        v[c] = val;
      }
    }
    buf ^= (NW > 1);
  }
  if (t == 0) out[blockIdx.x] = v[0];
}

template <int NW, int C>
void launch(const CrrTree* trees, const double* sf, int N, uint32_t n, double* out, hipStream_t s) {
  hipLaunchKernelGGL((crr_kernel<NW, C>), dim3(n), dim3(64 * NW), 0, s, trees, sf, N, out);
}

}  // namespace

int launch_crr(const CrrTree* trees_dev, const double* spot_factors_dev, int steps, uint32_t n_trees,
               double* out_dev, hipStream_t s) {
  const int nodes = steps + 1;
  if (steps <= HH_CRR_FORM_A_MAX_STEPS) {
    if (nodes <= 64) launch<1, 1>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else if (nodes <= 128) launch<1, 2>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else if (nodes <= 256) launch<1, 4>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else if (nodes <= 512) launch<1, 8>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else if (nodes <= 1024) launch<1, 16>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else launch<1, 32>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
  } else {
    if (nodes <= 4096) launch<16, 4>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else if (nodes <= 8192) launch<16, 8>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else if (nodes <= 16384) launch<16, 16>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
    else launch<16, 33>(trees_dev, spot_factors_dev, steps, n_trees, out_dev, s);
  }
  return (int)hipGetLastError();
}

}  // namespace hh

static_assert(sizeof(hh::CrrTree) == 8 * sizeof(double), "CrrTree is staged as 8 doubles");
static_assert(HH_CRR_MAX_STEPS + 1 <= 1024 * 33, "form B holds 33 registers per lane");
static_assert(HH_CRR_FORM_A_MAX_STEPS + 1 <= 64 * 32, "form A holds 32 registers per lane");

int hh_crr_solve(hh_ctx* ctx, int32_t steps, uint32_t n_trees, const double* forwards, const double* strikes,
                 const double* cps, const double* ups, const double* discounts, const int32_t* styles,
                 const double* spot_factors, uint32_t n_spot_rows, const uint32_t* spot_row_of_tree,
                 double* prices_out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!forwards || !strikes || !cps || !ups || !discounts || !styles || !prices_out)
    return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: NULL argument");
  if (steps < 1 || steps > HH_CRR_MAX_STEPS)
    return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: steps %d outside 1 .. %d", steps, HH_CRR_MAX_STEPS);
  if (n_trees == 0 || n_trees > (1u << 20))
    return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: 1 .. 2^20 trees per call");
  bool any_spot = false;
  for (uint32_t k = 0; k < n_trees; ++k) {
    if (styles[k] != HH_CRR_EUROPEAN && styles[k] != HH_CRR_AMERICAN_FORWARD && styles[k] != HH_CRR_AMERICAN_SPOT)
      return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: tree %u: unknown style %d", k, styles[k]);
    any_spot |= styles[k] == HH_CRR_AMERICAN_SPOT;
  }
  if (any_spot) {
    if (!spot_factors || !spot_row_of_tree)
      return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: NULL spot factors for an HH_CRR_AMERICAN_SPOT tree");
    if (n_spot_rows == 0 || n_spot_rows > n_trees)
      return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: n_spot_rows %u outside 1 .. n_trees", n_spot_rows);
    for (uint32_t k = 0; k < n_trees; ++k)
      if (styles[k] == HH_CRR_AMERICAN_SPOT && spot_row_of_tree[k] >= n_spot_rows)
        return fail(ctx, HH_ERR_INVALID, "hh_crr_solve: tree %u: spot row %u >= n_spot_rows %u", k,
                    spot_row_of_tree[k], n_spot_rows);
  }
  const size_t n = n_trees, rows = any_spot ? n_spot_rows : 0, row_len = (size_t)steps;
  const size_t n_par = 8 * n, n_sf = rows * row_len;
  std::vector<double> host(n_par + n_sf);  // trees (hh::CrrTree, 8 doubles each) | spot-factor rows
  for (size_t k = 0; k < n; ++k) {
    hh::CrrTree tr{};
    tr.F = forwards[k];
    tr.K = strikes[k];
    tr.cp = cps[k];
    tr.u = ups[k];
    tr.p = 1.0 / (1.0 + ups[k]);  // p = 1 / (1 + u), cox_ross_rubinstein.jl:124
    tr.q = 1.0 - tr.p;
    tr.disc = discounts[k];
    tr.style = styles[k];
    tr.row = styles[k] == HH_CRR_AMERICAN_SPOT ? spot_row_of_tree[k] : 0;
    std::memcpy(host.data() + 8 * k, &tr, sizeof(tr));
  }
  if (n_sf) std::memcpy(host.data() + n_par, spot_factors, n_sf * sizeof(double));
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const double* dev = nullptr;
  int rc = stage_host(ctx, ctx->payoffs, n_par + n_sf + n, host.data(), n_par + n_sf, &dev);
  if (rc) return rc;
  double* out_dev = ctx->payoffs + n_par + n_sf;
  if (ctx->timing) HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][0], ctx->stream));
  HH_HIP(ctx, hh::launch_crr(reinterpret_cast<const hh::CrrTree*>(dev), n_sf ? dev + n_par : nullptr, steps,
                             n_trees, out_dev, ctx->stream));
  if (ctx->timing) {
    HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][1], ctx->stream));
    ++ctx->t_count;
  }
  HH_HIP(ctx, hipMemcpyAsync(prices_out, out_dev, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return release_host_operands(ctx);
}
