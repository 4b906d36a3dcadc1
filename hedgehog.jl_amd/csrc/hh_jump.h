// The jump count and the jump sum of the Merton model (include/hedgehog_mc.h, "Merton (1976) jump diffusion"): a Poisson
// variate by inversion of one uniform and the sum of its jumps from one normal, as functions the device kernels
// (hh_jump.hip, hh_bates.hip) and a host program share — a host compiler sees nothing of HIP in it, so that
// tests/c/jump_host_check.cpp can hold it to a 50-digit restatement and run it under the host sanitizers — and, for
// hipcc alone, the path kernels' per-step jump on their own draws.  Internal; the public surface is
// include/hedgehog_mc.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

#if defined(__HIPCC__)
#include "hh_rng.h"
#define HH_JUMP_HD __host__ __device__
#else
#define HH_JUMP_HD
#endif

namespace hh {

// The jump parameters of a launch, passed BY VALUE beside SimArgs (wave-uniform: scalar registers).
struct JumpArgs {
  double mean;     // Poisson mean of one draw: λ·T (terminal law), λ·dt (path form)
  double p0;       // exp(-mean), formed on the host once per call
  double mu_j;     // mean of one jump in log S
  double sigma_j;  // standard deviation of one jump
};

// The smallest n with u <= c_n, c_0 = p0, p_k = p_{k-1}·m/k, c_k = c_{k-1} + p_k (one rounded operation each, in this
// order); HH_JUMP_MAX_COUNT at the latest.  The cap is a condition of the loop, not a tuning knob: the cumulative sum
// saturates in fp64 (m = 2.5: at 1 - 2^-52, below the largest uniform 1 - 2^-53), and a search bounded by the data alone
// would then never end.  m = 0: p0 = 1, so n = 0 for every u.
HH_JUMP_HD inline uint32_t poisson_inverse(double u, double m, double p0) {
  double p = p0, c = p0;
  for (uint32_t k = 1; k <= (uint32_t)HH_JUMP_MAX_COUNT; ++k) {
    if (u <= c) return k - 1u;
    p = p * m / (double)k;
    c = c + p;
  }
  return (uint32_t)HH_JUMP_MAX_COUNT;
}

// the jump sum of N > 0 jumps from one standard normal: N(N·μ_J, N·σ_J²)
HH_JUMP_HD inline __attribute__((always_inline)) double jump_sum(const JumpArgs& j, uint32_t N, double z) {
  const double n = (double)N;
  return fma(j.sigma_j * sqrt(n), z, n * j.mu_j);
}

#if defined(__HIPCC__)
// The path kernels' part (hh_jump.hip, hh_bates.hip), on the draws of domain kDomJump under the trajectory's key.
//
// The uniforms of the jump counts: block (h, 0, 0, kDomJump) serves steps 2h and 2h + 1 — words 0, 1 the even step,
// words 2, 3, carried here, the odd one: one block per two steps whatever n_steps is, an odd n_steps leaving the last
// block half read.
struct JumpUniforms {
  uint32_t odd_lo = 0u, odd_hi = 0u;
  __device__ __forceinline__ double even(uint32_t h, uint32_t k0, uint32_t k1) {
    const Philox4 b = philox4x32_10(h, 0u, 0u, kDomJump, k0, k1);
    odd_lo = b.c2;
    odd_hi = b.c3;
    return u01_fast(b.c0, b.c1);
  }
  __device__ __forceinline__ double odd() const { return u01_fast(odd_lo, odd_hi); }
};

// The jump of step k, after the step and before the date: the count N from the uniform u and, only where N > 0, the
// jump from the first normal of block (k, 1, 0, kDomJump), added to the log spot x; the mirror xa takes the same N and
// −z.  The search and the N > 0 branch diverge: the block is drawn by the rare lane that jumps — a branch, not a select
// over a block every lane would pay for.
template <bool ANTI>
__device__ __forceinline__ void jump_step(const JumpArgs& j, uint64_t key, uint32_t k, double u, double& x, double& xa) {
  const uint32_t N = poisson_inverse(u, j.mean, j.p0);
  if (N > 0u) {
    double z, unused;
    normal_pair(key, k, 1u, 0u, kDomJump, z, unused);
    x = x + jump_sum(j, N, z);
    if constexpr (ANTI) xa = xa + jump_sum(j, N, -z);
  }
}
#endif

// The host's part.  exp(μ_J + σ_J²/2) − 1 (expm1: exact 0 for μ_J = σ_J = 0, no cancellation for small jumps) …
inline double kappa_bar(const hh_jump& jump) { return expm1(jump.mu_j + 0.5 * jump.sigma_j * jump.sigma_j); }
// … λ·κ̄, the drift's compensator, as every launcher forms it
inline double merton_compensator(const hh_jump& jump) { return jump.lambda * kappa_bar(jump); }

// the parameters of a launch whose one Poisson draw covers `span` (T, or T/n_steps)
inline JumpArgs jump_args(const hh_jump& jump, double span) {
  JumpArgs j{};
  j.mean = jump.lambda * span;
  j.p0 = exp(-j.mean);
  j.mu_j = jump.mu_j;
  j.sigma_j = jump.sigma_j;
  return j;
}

}  // namespace hh
