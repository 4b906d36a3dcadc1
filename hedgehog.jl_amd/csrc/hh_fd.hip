// Crank–Nicolson finite differences for the Black–Scholes equation in log-spot, on the device: European and
// American vanillas, a basket of grids in one launch (hh_fd_solve, include/hedgehog_mc.h).  DESIGN §5.11.
//
// The scheme is the one hh_fd.h states serially.  A time step is a tridiagonal solve with CONSTANT coefficients, so
// everything of the factorisation — pivots, elimination multipliers, substitution multipliers — depends on the phase
// (k, θ) alone: it is formed when a phase starts (Rannacher half steps, then Crank–Nicolson), never per step.  Only
// right-hand sides move.  Both sweeps are first-order recurrences and both are scanned:
//   elimination   y_q = al_q·y_{q+1} + d_q                     (affine, from the far end towards the spot-side end)
//   substitution  V_q = max(as_q·V_{q−1} + d'_q, g_q)          (max-affine, the other way; European: g = −1e300)
// Internal index q = 0 … M − 2 runs over the interior nodes in the direction of the substitution: j = q + 1 for a
// put, j = M − 1 − q for a call (the mirrored solve, lo and up exchanged) — one code path prices both.  Thread t
// holds nodes q = t·C … t·C + C − 1 in registers.  One scan is a local pass (the lane's composite map), a Kogge–Stone
// scan over the 64 lanes by __shfl (its multiplier products are constants of the phase as well), between the waves
// of a workgroup a serial fold of the NW wave totals through LDS, and a second local pass from the lane's incoming
// value.  Slots q >= M − 1 are padding: al = as = 1/pivot = 0, g = 0, right-hand side 0, so they hold 0.
//   form A  M <= HH_FD_FORM_A_MAX_SPACE: one wave per option, C in {1, 2, 4, 8, 16};
//   form B  larger M: four waves per option, C in {8, 16}.
// The form depends on M alone, and an option reads nothing but its own record: the same bits alone, in a basket, at
// any position.  Every loop is bounded by M, N or C, whatever the scalars hold.
#include <cmath>
#include <cstring>
#include <vector>

#include "hh_ctx.h"
#include "hh_fd.h"

#pragma clang fp contract(off)

namespace hh {

namespace {

constexpr double kNoExercise = -1e300;  // a European node's "payoff" in the max-affine maps: below every value

template <int NW, int C>
__global__ __launch_bounds__(64 * NW) void fd_kernel(const FdOption* __restrict__ opts, int M, int N, int R,
                                                     uint32_t n_options, double* __restrict__ out) {
  constexpr int WG = 64 * NW;
  __shared__ double piv_s[WG * C];  // the pivots of the phase being set up, by q
  __shared__ double wtot[5][NW];    // wave totals: P, T (elimination) | A, B, G (substitution)
  __shared__ double edge[2][NW];    // V of a wave's first and last slot
  __shared__ double res[3];
  const FdOption o = opts[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nI = M - 1, half = M / 2;
  const bool call = o.cp > 0.0, am = o.style == HH_FD_AMERICAN;
  const FdCoef co{o.lo, o.di, o.up};
  const double cm = call ? o.up : o.lo;  // couples q − 1
  const double cq = call ? o.lo : o.up;  // couples q + 1

  auto spot = [&](int q) {  // q = −1 and q = nI are the Dirichlet ends
    const int j = call ? M - 1 - q : q + 1;
    return exp(o.x0 + (double)(j - half) * o.h);
  };
  auto payoff = [&](double S) { return fmax(o.cp * (S - o.K), 0.0); };

  double V[C], g[C], al[C], as[C], ip[C], d[C];
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const int q = t * C + i;
    const double pay = q < nI ? payoff(spot(q)) : 0.0;
    V[i] = pay;
    g[i] = q < nI ? (am ? pay : kNoExercise) : 0.0;
    al[i] = as[i] = ip[i] = d[i] = 0.0;
  }
  const double SB = spot(-1);
  double VB = payoff(SB), VT = payoff(spot(nI));
  if constexpr (NW > 1) {
    if (lane == 0) edge[0][w] = V[0];
    if (lane == 63) edge[1][w] = V[C - 1];
    __syncthreads();
  }

  const double dt = o.T / (double)N;
  double tau = 0.0;
  double Pl[6], Al[6], Pinc = 0.0, Ainc = 0.0, Pnext = 0.0;
  FdPhase ph{0.0, 1.0, 0.0, 0.0};
  double k = dt;
  for (int step = 0; step < N; ++step) {
    const bool rann = step < R;
    if (step == 0 || step == R) {
      // ---- a phase starts: pivots (the same serial recurrence in every thread; it stops early once it repeats
      // itself to the bit, from where it is constant), then this thread's multipliers and the scans' products
      k = rann ? 0.5 * dt : dt;
      ph = fd_phase(FdCoef{cm, o.di, cq}, k, rann ? 1.0 : 0.5);
      __syncthreads();
      double piv = ph.B;
      if (t == 0) piv_s[nI - 1] = piv;
      int qq = nI - 2;
      for (; qq >= 0; --qq) {
        const double m = ph.C / piv;
        const double np = ph.B - m * ph.A;
        if (np == piv) break;
        piv = np;
        if (t == 0) piv_s[qq] = piv;
      }
      for (int f = t; f <= qq; f += WG) piv_s[f] = piv;
      __syncthreads();
      double prodP = 1.0, prodA = 1.0;
#pragma unroll
      for (int i = 0; i < C; ++i) {
        const int q = t * C + i;
        al[i] = q + 1 < nI ? ph.C / piv_s[q + 1] : 0.0;
        ip[i] = q < nI ? 1.0 / piv_s[q] : 0.0;
        as[i] = ph.A * ip[i];
        prodP = prodP * al[i];
        prodA = prodA * as[i];
      }
#pragma unroll
      for (int lv = 0; lv < 6; ++lv) {
        const int s = 1 << lv;
        Pl[lv] = prodP;
        Al[lv] = prodA;
        const double pn = __shfl_down(prodP, s, 64);
        const double an = __shfl_up(prodA, s, 64);
        if (lane + s < 64) prodP = prodP * pn;
        if (lane >= s) prodA = prodA * an;
      }
      Pinc = prodP;
      Ainc = prodA;
      Pnext = __shfl_down(Pinc, 1, 64);
      if constexpr (NW > 1) {
        if (lane == 0) wtot[0][w] = Pinc;
        if (lane == 63) wtot[2][w] = Ainc;
        __syncthreads();
      }
    }
    const int sub = rann ? 2 : 1;
    for (int hs = 0; hs < sub; ++hs) {
      // ---- right-hand side from the old values
      if (ph.e != 0.0) {
        double vlo = __shfl_up(V[C - 1], 1, 64);
        double vhi = __shfl_down(V[0], 1, 64);
        if constexpr (NW > 1) {
          if (lane == 0) vlo = w > 0 ? edge[1][w > 0 ? w - 1 : 0] : VB;
          if (lane == 63) vhi = w + 1 < NW ? edge[0][w + 1 < NW ? w + 1 : 0] : 0.0;
        } else {
          if (lane == 0) vlo = VB;
          if (lane == 63) vhi = 0.0;
        }
#pragma unroll
        for (int i = 0; i < C; ++i) {
          const int q = t * C + i;
          const double vm = i > 0 ? V[i > 0 ? i - 1 : 0] : vlo;
          double vp = i + 1 < C ? V[i + 1 < C ? i + 1 : 0] : vhi;
          if (q + 1 == nI) vp = VT;
          const double below = call ? vp : vm, above = call ? vm : vp;  // V_{j−1}, V_{j+1}
          d[i] = q < nI ? fd_rhs(co, ph.e, below, V[i], above) : 0.0;
        }
      } else {
#pragma unroll
        for (int i = 0; i < C; ++i) d[i] = V[i];
      }
      tau = tau + k;
      const double VBn = (am && !call) ? o.K - SB : o.cp * (SB - o.K * exp(-o.r * tau));  // the far end stays 0

      // ---- elimination: y_q = al_q·y_{q+1} + d_q, scanned from the far end
      double T = 0.0;
#pragma unroll
      for (int i = C - 1; i >= 0; --i) T = al[i] * T + d[i];
#pragma unroll
      for (int lv = 0; lv < 6; ++lv) {
        const int s = 1 << lv;
        const double tn = __shfl_down(T, s, 64);
        if (lane + s < 64) T = Pl[lv] * tn + T;
      }
      double y = __shfl_down(T, 1, 64);
      if (lane == 63) y = 0.0;
      if constexpr (NW > 1) {
        if (lane == 0) wtot[1][w] = T;
        __syncthreads();
        double Y = 0.0;
        for (int ww = NW - 1; ww > w; --ww) Y = wtot[0][ww] * Y + wtot[1][ww];
        y = lane == 63 ? Y : Pnext * Y + y;
      }
#pragma unroll
      for (int i = C - 1; i >= 0; --i) {
        y = al[i] * y + d[i];
        d[i] = y * ip[i];
      }

      // ---- substitution with exercise: V_q = max(as_q·V_{q−1} + d_q, g_q), scanned from the near end
      double Bv = 0.0, Gv = kNoExercise;
#pragma unroll
      for (int i = 0; i < C; ++i) {
        Gv = fmax(as[i] * Gv + d[i], g[i]);
        Bv = as[i] * Bv + d[i];
      }
#pragma unroll
      for (int lv = 0; lv < 6; ++lv) {
        const int s = 1 << lv;
        const double bn = __shfl_up(Bv, s, 64);
        const double gn = __shfl_up(Gv, s, 64);
        if (lane >= s) {
          Gv = fmax(Al[lv] * gn + Bv, Gv);
          Bv = Al[lv] * bn + Bv;
        }
      }
      double X = VBn;  // what enters this wave
      if constexpr (NW > 1) {
        if (lane == 63) {
          wtot[3][w] = Bv;
          wtot[4][w] = Gv;
        }
        __syncthreads();
        for (int ww = 0; ww < w; ++ww) X = fmax(wtot[2][ww] * X + wtot[3][ww], wtot[4][ww]);
      }
      const double xout = fmax(Ainc * X + Bv, Gv);
      double x = __shfl_up(xout, 1, 64);
      if (lane == 0) x = X;
#pragma unroll
      for (int i = 0; i < C; ++i) {
        x = fmax(as[i] * x + d[i], g[i]);
        V[i] = x;
      }
      VB = VBn;
      VT = 0.0;
      if constexpr (NW > 1) {
        if (lane == 0) edge[0][w] = V[0];
        if (lane == 63) edge[1][w] = V[C - 1];
        __syncthreads();
      }
    }
  }

  // ---- price, delta and gamma from the three nodes round the spot
  const int qc = half - 1;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const int q = t * C + i;
    if (q >= qc - 1 && q <= qc + 1) res[q - (qc - 1)] = V[i];
  }
  __syncthreads();
  if (t == 0) {
    const double vdn = call ? res[2] : res[0], vc = res[1], vup = call ? res[0] : res[2];
    const double d1 = (vup - vdn) / (2.0 * o.h);
    const double d2 = ((vup - 2.0 * vc) + vdn) / (o.h * o.h);
    out[blockIdx.x] = vc;
    out[(size_t)n_options + blockIdx.x] = d1 / o.S0;
    out[2 * (size_t)n_options + blockIdx.x] = (d2 - d1) / (o.S0 * o.S0);
  }
}

template <int NW, int C>
void launch(const FdOption* opts, int M, int N, int R, uint32_t n, double* out, hipStream_t s) {
  hipLaunchKernelGGL((fd_kernel<NW, C>), dim3(n), dim3(64 * NW), 0, s, opts, M, N, R, n, out);
}

}  // namespace

// a form holds the M − 1 interior nodes and at least one padding slot: M <= 64·NW·C
int launch_fd(const FdOption* opts_dev, int M, int N, int R, uint32_t n_options, double* out_dev, hipStream_t s) {
  if (M <= 64) launch<1, 1>(opts_dev, M, N, R, n_options, out_dev, s);
  else if (M <= 128) launch<1, 2>(opts_dev, M, N, R, n_options, out_dev, s);
  else if (M <= 256) launch<1, 4>(opts_dev, M, N, R, n_options, out_dev, s);
  else if (M <= 512) launch<1, 8>(opts_dev, M, N, R, n_options, out_dev, s);
  else if (M <= HH_FD_FORM_A_MAX_SPACE) launch<1, 16>(opts_dev, M, N, R, n_options, out_dev, s);
  else if (M <= 2048) launch<4, 8>(opts_dev, M, N, R, n_options, out_dev, s);
  else launch<4, 16>(opts_dev, M, N, R, n_options, out_dev, s);
  return (int)hipGetLastError();
}

}  // namespace hh

static_assert(sizeof(hh::FdOption) == 11 * sizeof(double), "FdOption is staged as 11 doubles");
static_assert(HH_FD_FORM_A_MAX_SPACE == 64 * 16, "form A holds 16 nodes per lane");
static_assert(HH_FD_MAX_SPACE <= 256 * 16, "form B holds 16 nodes per thread");

int hh_fd_solve(hh_ctx* ctx, int32_t space_steps, int32_t time_steps, int32_t rannacher_steps, uint32_t n_options,
                const double* spots, const double* strikes, const double* cps, const double* sigmas,
                const double* rates, const double* expiries, const double* half_widths, const int32_t* styles,
                double* prices_out, double* deltas_out, double* gammas_out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!spots || !strikes || !cps || !sigmas || !rates || !expiries || !half_widths || !styles || !prices_out)
    return fail(ctx, HH_ERR_INVALID, "hh_fd_solve: NULL argument");
  const int M = space_steps, N = time_steps, R = rannacher_steps;
  if (M < 4 || M > HH_FD_MAX_SPACE || (M & 1))
    return fail(ctx, HH_ERR_INVALID, "hh_fd_solve: space_steps %d not an even number in 4 .. %d", M, HH_FD_MAX_SPACE);
  if (N < 1 || N > HH_FD_MAX_TIME)
    return fail(ctx, HH_ERR_INVALID, "hh_fd_solve: time_steps %d outside 1 .. %d", N, HH_FD_MAX_TIME);
  if (R < 0 || R > N)
    return fail(ctx, HH_ERR_INVALID, "hh_fd_solve: rannacher_steps %d outside 0 .. time_steps", R);
  if (n_options == 0 || n_options > (1u << 20))
    return fail(ctx, HH_ERR_INVALID, "hh_fd_solve: 1 .. 2^20 options per call");
  const size_t n = n_options, n_par = 11 * n;
  std::vector<double> host(n_par);
  for (size_t i = 0; i < n; ++i) {
    if (styles[i] != HH_FD_EUROPEAN && styles[i] != HH_FD_AMERICAN)
      return fail(ctx, HH_ERR_INVALID, "hh_fd_solve: option %zu: unknown style %d", i, styles[i]);
    hh::FdOption o{};
    o.S0 = spots[i];
    o.K = strikes[i];
    o.cp = cps[i];
    o.r = rates[i];
    o.T = expiries[i];
    o.h = half_widths[i] / (double)(M / 2);
    o.x0 = std::log(spots[i]);
    const hh::FdCoef c = hh::fd_coef(sigmas[i], rates[i], o.h);
    if (!hh::fd_coef_ok(c))
      return fail(ctx, HH_ERR_INVALID,
                  "hh_fd_solve: option %zu: lo = %g, up = %g are not both positive (more space steps are needed)", i,
                  c.lo, c.up);
    o.lo = c.lo;
    o.di = c.di;
    o.up = c.up;
    o.style = styles[i];
    std::memcpy(host.data() + 11 * i, &o, sizeof(o));
  }
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const double* dev = nullptr;
  int rc = stage_host(ctx, ctx->payoffs, n_par + 3 * n, host.data(), n_par, &dev);
  if (rc) return rc;
  double* out_dev = ctx->payoffs + n_par;
  if (ctx->timing) HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][0], ctx->stream));
  HH_HIP(ctx, hh::launch_fd(reinterpret_cast<const hh::FdOption*>(dev), M, N, R, n_options, out_dev, ctx->stream));
  if (ctx->timing) {
    HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][1], ctx->stream));
    ++ctx->t_count;
  }
  HH_HIP(ctx, hipMemcpyAsync(prices_out, out_dev, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (deltas_out)
    HH_HIP(ctx, hipMemcpyAsync(deltas_out, out_dev + n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (gammas_out)
    HH_HIP(ctx, hipMemcpyAsync(gammas_out, out_dev + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return release_host_operands(ctx);
}
