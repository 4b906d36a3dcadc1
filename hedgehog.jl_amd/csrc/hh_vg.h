// The gamma variate and the increment of the Variance Gamma model (include/hedgehog_mc.h, "Variance Gamma"): Marsaglia
// and Tsang's (2000) rejection sampler with the shape boost for a < 1, as a function of a DRAW SOURCE — the device kernels
// (hh_vg.hip) feed it Philox blocks under the trajectory's key, a host program (tests/c/vg_host_check.cpp) draws of its
// choosing, so that the sampler can be held to a 50-digit restatement and run under the host sanitizers.  A host
// compiler sees nothing of HIP in it.  Internal; the public surface is include/hedgehog_mc.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

#if defined(__HIPCC__)
#define HH_VG_HD __host__ __device__
#else
#define HH_VG_HD
#endif

namespace hh {

// The parameters of a launch whose one gamma draw covers `span` (T, or T/n_steps), passed BY VALUE beside SimArgs
// (wave-uniform: scalar registers).  Formed on the host once per call by vg_args, below.
struct VgArgs {
  double d, c;    // d = a' − 1/3, c = 1/sqrt(9d), a' = a + 1 when boosted, else a; a = span/ν the shape
  double inv_a;   // 1/a: the exponent of the boost's uniform
  double nu_d;    // ν·d: an accepted proposal v is the variate ν·d·v
  double theta;   // θ
  double drift;   // (r + ω)·span
  int32_t boost;  // a < 1
  int32_t pad_;
};

// One attempt's draws, as a source hands them out: the proposal's standard normal z, the acceptance uniform U and the
// boost's uniform U′ (read only when VgArgs::boost), both in (0, 1).
struct VgDraws {
  double z, u, u_boost;
};

// Gamma(shape a, scale ν).  Attempt t = 0, 1, …: the source's draws of attempt t, then
//   x = 1 + c·z,  v = (x·x)·x;  only where v > 0:  rhs = (((0.5·z)·z + d) − d·v) + d·log v,
//   val = (ν·d)·v, boosted: val·exp(log(U′)·(1/a));  accepted when log U < rhs
// — one rounded fp64 operation each, in this order.  The loop ends after HH_VG_MAX_ATTEMPTS attempts at the latest with
// the value of the last proposal that had v > 0 (+0 when none had): the cap is a condition of the loop, not a tuning
// knob — an acceptance is at least 0.95 likely whatever the shape, but a loop bounded by the draws alone has no bound.
// The boosted product may underflow to +0 (a = 0.008: 0.3 % of the draws); the increment is then the drift alone.
// *attempts (nullable): how many attempts were made.
template <class Source>
HH_VG_HD inline double gamma_mt(const VgArgs& g, Source& src, uint32_t* attempts = nullptr) {
  double last = 0.0;
  uint32_t t = 0u;
  for (; t < (uint32_t)HH_VG_MAX_ATTEMPTS; ++t) {
    const VgDraws w = src.attempt(t);
    const double x = 1.0 + g.c * w.z;
    const double v = (x * x) * x;
    if (v > 0.0) {
      const double rhs = (((0.5 * w.z) * w.z + g.d) - g.d * v) + g.d * log(v);
      double val = g.nu_d * v;
      if (g.boost) val = val * exp(log(w.u_boost) * g.inv_a);
      last = val;
      if (log(w.u) < rhs) {
        ++t;
        break;
      }
    }
  }
  if (attempts) *attempts = t;
  return last;
}

// The increment of log S over the span, from the gamma variate g and a standard normal z independent of it:
// (drift + θ·g) + (σ·sqrt(g))·z, one rounded operation each in this order; the antithetic mirror takes the same g and −z.
// sqrt is the correctly rounded one (g = +0 gives 0: the drift alone).
HH_VG_HD inline __attribute__((always_inline)) double vg_increment(const VgArgs& v, double sigma, double g, double z) {
  return (v.drift + v.theta * g) + (sigma * sqrt(g)) * z;
}

// The host's part.  ω = log(1 − θν − σ²ν/2)/ν, the drift's compensator: e^{−rt}·S is a martingale.  Each a single rounded
// operation in this order; the entry points have checked that the logarithm's argument is positive.
inline double vg_moment_arg(double sigma, const hh_vg& vg, double p) {  // 1 − θν·p − σ²ν·p²/2: E exp(p·X_t) is finite iff > 0
  return (1.0 - (vg.theta * vg.nu) * p) - ((0.5 * (sigma * sigma)) * vg.nu) * (p * p);
}
inline double vg_omega(double sigma, const hh_vg& vg) { return log(vg_moment_arg(sigma, vg, 1.0)) / vg.nu; }

inline VgArgs vg_args(double sigma, double r_drift, const hh_vg& vg, double span) {
  VgArgs g{};
  const double a = span / vg.nu;
  g.boost = a < 1.0 ? 1 : 0;
  const double a1 = g.boost ? a + 1.0 : a;
  g.d = a1 - 1.0 / 3.0;
  g.c = 1.0 / sqrt(9.0 * g.d);
  g.inv_a = 1.0 / a;
  g.nu_d = vg.nu * g.d;
  g.theta = vg.theta;
  g.drift = (r_drift + vg_omega(sigma, vg)) * span;
  return g;
}

}  // namespace hh
