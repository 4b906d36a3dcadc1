// The Andersen–Broadie dual upper bound of an exercise policy on Heston Euler paths (include/hedgehog_mc.h, "Dual bounds
// for American exercise").  Two kernels on the (log S, V) rows [n_dates + 1][2][n_outer] of a plain outer walk:
//
//   nested_continuation_kernel  Ĉ[t][i], the value of CONTINUING under the policy from the stored state of date t and outer
//                               column i, by n_inner fresh walks — the heaviest launch of the library: outer columns × dates
//                               × inner walks × remaining steps;
//   dual_outer_kernel           the martingale M_t built from Ĉ and the policy's decisions, and max_t (D^t·max(pay_t, 0) − M_t)
//                               per outer column.
//
// NESTED: one wave per (t, i), lanes striding the inner walks j = lane, lane + 64, … (n_inner is a multiple of 64).  A lane
// sets HestonModel's state to the stored (x, v) — init supplies whatever else a state holds — and walks steps t·m .. n_steps − 1
// with hh_sim.h's step and euler_pair_increments: the outer walk's arithmetic, statement for statement.  On every m-th step it
// evaluates the policy (one date, one wave-uniform block of 4 + B doubles: scalar loads) with hh_lsm_basis.h's lsm_phi in the
// induction's order.  A lane that has stopped keeps stepping — its state is not read again — so the wave never diverges; the
// wave leaves a batch's date loop when no lane is still walking (one ballot per date).  Σy and Σy² of the lanes go down the
// shuffle tree of hh_reduce.h's tree256 (offsets 32, 16, …, 1: a fixed order), lane 0 writes Ĉ and its standard error with
// ordinary stores.  No atomics, no LDS, no scratch; the same inputs give the same bits.
//
// GRID ORDER: wave w = t·n_outer + i, so the workgroups of t = 0 — the longest walks, n_steps steps — are dispatched first
// and those of t = n_dates − 1 — m steps — last.  The dispatcher hands a workgroup to whichever CU frees a slot, so the launch
// ends when the LAST workgroups end: with the short walks there the tail in which CUs idle is a fraction of one short walk;
// in the opposite order it would be most of a full-length walk on a nearly empty chip.
//
// INNER KEYS (stated in the header): key = mix(mix(inner_seed + φ·(i + 1)) ^ (t·2^32 + j)), the draws of step s at Philox counter
// (s + 2^31, 0, 0, 0) — an outer walk uses (s, 0, 0, 0), s < 2^31, so no inner draw repeats an outer one whatever the seeds.
#include "hh_kernels.h"
#include "hh_lsm_basis.h"
#include "hh_sim.h"

namespace hh {
namespace {

constexpr int kWavesPerWg = 4;
constexpr uint32_t kInnerCounter = 0x80000000u;

struct BoundsArgs {
  SimArgs<0> a;            // the outer walk's block (make_args0): the step's constants, cp, strike
  const double* rows;      // [n_dates + 1][2][n_outer]
  const double* policy;    // [n_dates + 1][4 + B]
  const double* disc_pow;  // [k] = D^k
  uint64_t inner_seed;
  uint32_t n_outer, n_dates, every, n_inner;
  int32_t B, p;            // p: the degree
  uint32_t expo[kLsmBasisPad];
};

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the policy's fitted value of date `t` at (S, v): the induction's φ·c on the descriptor HH_LSM_STATES_LOG_SPOT_VARIANCE
__device__ __forceinline__ double policy_fit(const BoundsArgs& b, uint32_t t, double S, double v) {
  constexpr int P = lsm_max_degree(2);
  const double* __restrict__ pol = b.policy + (size_t)t * (4 + b.B);  // uniform
  const double z[2] = {(S - pol[0]) * pol[2], (v - pol[1]) * pol[3]};
  double fit = pol[4] * lsm_phi<2, P>(1.0, z, b.expo[0], b.p);
  for (int j = 1; j < b.B; ++j) fit = fma(pol[4 + j], lsm_phi<2, P>(1.0, z, b.expo[j], b.p), fit);
  return fit;
}

__device__ __forceinline__ double wave_sum_down(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;  // lane 0 holds the sum
}

template <bool SPLIT>
__global__ __launch_bounds__(64 * kWavesPerWg) void nested_continuation_kernel(const BoundsArgs b, double* __restrict__ cont,
                                                                               double* __restrict__ cont_se) {
  using M = HestonModel<0, SPLIT>;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * kWavesPerWg + (threadIdx.x >> 6);
  if (w >= (uint64_t)b.n_dates * b.n_outer) return;  // a whole wave
  const uint32_t t = (uint32_t)(w / b.n_outer), i = (uint32_t)(w % b.n_outer);
  const double x0 = b.rows[((size_t)t * 2) * b.n_outer + i], v0 = b.rows[((size_t)t * 2 + 1) * b.n_outer + i];
  const uint64_t ki = mix64(b.inner_seed + 0x9E3779B97F4A7C15ull * ((uint64_t)i + 1ull));
  double sy = 0.0, syy = 0.0;
  for (uint32_t j = lane; j < b.n_inner; j += 64u) {  // n_inner % 64 == 0: every lane takes every batch
    const uint64_t key = mix64(ki ^ (((uint64_t)t << 32) | (uint64_t)j));
    typename M::State st;
    M::init(st, b.a);
    st.x.v = x0;
    st.v.v = v0;
    bool walking = true;
    double y = 0.0;
    for (uint32_t d = t + 1; d <= b.n_dates; ++d) {
      uint32_t s = (d - 1) * b.every;
      for (uint32_t k = 0; k < b.every; ++k, ++s) {
        double d1, d2;
        euler_pair_increments(key, s | kInnerCounter, b.a, d1, d2);
        M::step(st, b.a, d1, d2);
      }
      const double S = exp(st.x.v);
      const double pay = b.a.cp * (S - b.a.strike.v);
      bool stop = true;
      double val = pay > 0.0 ? pay : 0.0;
      if (d < b.n_dates) {  // uniform
        stop = pay > 0.0 && pay > policy_fit(b, d, S, st.v.v);
        val = pay;
      }
      if (walking && stop) {
        y = b.disc_pow[d - t] * val;
        walking = false;
      }
      if (__ballot(walking) == 0ull) break;  // uniform: nobody is still walking
    }
    sy += y;
    syy = fma(y, y, syy);
  }
  sy = wave_sum_down(sy);
  syy = wave_sum_down(syy);
  if (lane == 0) {
    const double n = (double)b.n_inner, mean = sy / n;
    const double ss = syy - n * mean * mean;
    cont[w] = mean;
    cont_se[w] = sqrt((ss > 0.0 ? ss : 0.0) / (n * (n - 1.0)));
  }
}

// One lane per outer column: the recursion of the header.  cont: [n_dates][n_outer].
__global__ __launch_bounds__(256) void dual_outer_kernel(const BoundsArgs b, const double* __restrict__ cont,
                                                         double* __restrict__ pathwise_max) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.n_outer) return;
  const size_t n = b.n_outer;
  const double pay0 = b.a.cp * (exp(b.rows[i]) - b.a.strike.v);
  double best = pay0 > 0.0 ? pay0 : 0.0, mart = 0.0, c_prev = cont[i];
  for (uint32_t t = 1; t <= b.n_dates; ++t) {
    const double x = b.rows[((size_t)t * 2) * n + i], v = b.rows[((size_t)t * 2 + 1) * n + i];
    const double S = exp(x);
    const double pay = b.a.cp * (S - b.a.strike.v), payp = pay > 0.0 ? pay : 0.0;
    double L = payp, c_here = 0.0;
    if (t < b.n_dates) {  // uniform
      c_here = cont[(size_t)t * n + i];
      L = pay > 0.0 && pay > policy_fit(b, t, S, v) ? pay : c_here;
    }
    const double dt = b.disc_pow[t];
    mart = (mart + dt * L) - b.disc_pow[t - 1] * c_prev;
    const double gap = dt * payp - mart;
    best = gap > best ? gap : best;
    c_prev = c_here;
  }
  pathwise_max[i] = best;
}

BoundsArgs bounds_args(const hh_model& m, const hh_config& c, const BoundsLaunch& l) {
  BoundsArgs b{};
  b.a = make_args0(m, c, DevicePtrs{});
  b.rows = l.rows; b.policy = l.policy; b.disc_pow = l.disc_pow; b.inner_seed = l.inner_seed;
  b.n_outer = (uint32_t)c.n_paths; b.n_dates = l.n_dates; b.every = c.n_steps / l.n_dates; b.n_inner = l.n_inner;
  b.B = lsm_basis_fill(2, l.degree, b.expo);
  b.p = l.degree;
  return b;
}

}  // namespace

int launch_nested_continuation(const hh_model& m, const hh_config& c, const BoundsLaunch& l, double* cont, double* cont_se,
                               hipStream_t s) {
  const BoundsArgs b = bounds_args(m, c, l);
  const uint64_t waves = (uint64_t)b.n_dates * b.n_outer;
  if (b.B == 0 || b.every == 0 || b.n_inner == 0 || b.n_inner % 64u || waves == 0 || waves > 0x80000000ull)
    return (int)hipErrorInvalidValue;  // the entry point has refused it
  const dim3 grid((unsigned)((waves + kWavesPerWg - 1) / kWavesPerWg)), block(64 * kWavesPerWg);
  if (c.em_split) hipLaunchKernelGGL(nested_continuation_kernel<true>, grid, block, 0, s, b, cont, cont_se);
  else hipLaunchKernelGGL(nested_continuation_kernel<false>, grid, block, 0, s, b, cont, cont_se);
  return (int)hipGetLastError();
}

int launch_dual_outer(const hh_model& m, const hh_config& c, const BoundsLaunch& l, const double* cont, double* pathwise_max,
                      hipStream_t s) {
  const BoundsArgs b = bounds_args(m, c, l);
  if (b.B == 0 || b.n_outer == 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dual_outer_kernel, dim3((b.n_outer + 255u) / 256u), dim3(256), 0, s, b, cont, pathwise_max);
  return (int)hipGetLastError();
}

}  // namespace hh
