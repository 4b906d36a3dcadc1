// One step of Andersen's quadratic-exponential scheme for the Heston variance and log spot (include/hedgehog_mc.h,
// "Heston paths by the quadratic-exponential scheme" — every operation is stated there in this order), as functions the
// device kernels (hh_qe.hip, hh_bates.hip) and a host program share: a host compiler sees nothing of HIP in it, so that
// tests/c/qe_host_check.cpp can hold them to long-double evaluations and run them under the host sanitizers; for hipcc
// alone, the step of a trajectory and its mirror on their own draws (qe_pair_step).  Every operation is one rounded fp64
// operation (the library is built with -ffp-contract=off); sqrt, log and the divisions are the correctly rounded or
// 1-ulp ones of the language.  Internal; the public surface is include/hedgehog_mc.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

#if defined(__HIPCC__)
#include "hh_rng.h"
#define HH_QE_HD __host__ __device__
#else
#define HH_QE_HD
#endif

namespace hh {

// The constants of a launch, formed ONCE per call on the host (qe_args) and passed BY VALUE beside SimArgs
// (wave-uniform: scalar registers).
struct QeArgs {
  double E;       // exp(-κ·dt)
  double c1;      // σ²·E·(1 − E)/κ
  double c2;      // θ·σ²·(1 − E)²/(2κ)
  double th_ome;  // θ·(1 − E)
  double rdt;     // r·dt
  double K0, K1, K2, K3, K4;
  double A;       // K2 + K4/2
  double k13;     // K1 + K3/2
  double psi_c;   // the branch threshold, in [1, 2]
};

// The host's part, in the header's order.  dt = T/n_steps as the caller formed it.
inline QeArgs qe_args(double kappa, double theta, double sigma, double rho, double r, double dt, double psi_c) {
  QeArgs q;
  q.E = exp(-(kappa * dt));
  const double ome = 1.0 - q.E, s2 = sigma * sigma;
  q.c1 = ((s2 * q.E) * ome) / kappa;
  q.c2 = ((theta * s2) * (ome * ome)) / (2.0 * kappa);
  q.th_ome = theta * ome;
  q.rdt = r * dt;
  const double kr = (kappa * rho) / sigma, ros = rho / sigma;
  q.K0 = -((((rho * kappa) * theta) * dt) / sigma);
  const double h = (0.5 * dt) * (kr - 0.5);
  q.K1 = h - ros;
  q.K2 = h + ros;
  q.K3 = (0.5 * dt) * (1.0 - rho * rho);
  q.K4 = q.K3;
  q.A = q.K2 + 0.5 * q.K4;
  q.k13 = q.K1 + 0.5 * q.K3;
  q.psi_c = psi_c == 0.0 ? 1.5 : psi_c;
  return q;
}

// the moment match: m = E[v′ | v], ψ = Var[v′ | v]/m².  v >= 0 and th_ome > 0 (checked on the host): m > 0.
struct QeMoments {
  double m, psi;
};
HH_QE_HD inline QeMoments qe_moments(const QeArgs& q, double v) {
  QeMoments r;
  r.m = q.th_ome + v * q.E;
  const double s2 = v * q.c1 + q.c2;
  r.psi = s2 / (r.m * r.m);
  return r;
}

// ψ <= ψ_c <= 2: t = 2/ψ >= 1, so t − 1 >= 0 and both roots exist
struct QeQuad {
  double a, b2;
};
HH_QE_HD inline QeQuad qe_quad(const QeMoments& mo) {
  const double t = 2.0 / mo.psi;
  QeQuad s;
  s.b2 = (t - 1.0) + sqrt(t) * sqrt(t - 1.0);
  s.a = mo.m / (1.0 + s.b2);
  return s;
}
HH_QE_HD inline double qe_quad_next(const QeQuad& s, double zv) {
  const double bz = sqrt(s.b2) + zv;
  return s.a * (bz * bz);
}
// ln E exp(A·v′), A <= 0: 1 − 2Aa >= 1
HH_QE_HD inline double qe_quad_lnM(const QeQuad& s, double A) {
  const double d = 1.0 - (2.0 * A) * s.a;
  return ((A * s.b2) * s.a) / d - 0.5 * log(d);
}

// ψ > ψ_c >= 1: 0 < p < 1, β > 0
struct QeExp {
  double p, omp, beta;
};
HH_QE_HD inline QeExp qe_exp(const QeMoments& mo) {
  QeExp s;
  s.p = (mo.psi - 1.0) / (mo.psi + 1.0);
  s.omp = 1.0 - s.p;
  s.beta = s.omp / mo.m;
  return s;
}
HH_QE_HD inline double qe_exp_next(const QeExp& s, double U) {
  if (U <= s.p) return 0.0;
  return log(s.omp / (1.0 - U)) / s.beta;
}
// A <= 0: β − A >= β > 0
HH_QE_HD inline double qe_exp_lnM(const QeExp& s, double A) { return log(s.p + (s.beta * s.omp) / (s.beta - A)); }

// x′ from (x, v, v′): k0 is K0, or K0* = −ln M − (K1 + K3/2)·v under the martingale correction
HH_QE_HD inline double qe_k0_star(const QeArgs& q, double lnM, double v) { return -lnM - q.k13 * v; }
HH_QE_HD inline double qe_log_spot(const QeArgs& q, double x, double v, double vn, double k0, double zx) {
  const double drift = ((q.rdt + k0) + q.K1 * v) + q.K2 * vn;
  return (x + drift) + sqrt(q.K3 * v + q.K4 * vn) * zx;
}

// (x, v) -> (x′, v′) of one member: its own moments mo, its own normals and — exponential branch only — its own U
struct QeState {
  double x, v;
};
template <bool MART>
HH_QE_HD inline __attribute__((always_inline)) void qe_member_step(QeState& s, const QeArgs& q, const QeMoments& mo,
                                                                   bool quad, double zv, double zx, double U) {
  double vn, k0 = q.K0;
  if (quad) {
    const QeQuad b = qe_quad(mo);
    vn = qe_quad_next(b, zv);
    if constexpr (MART) k0 = qe_k0_star(q, qe_quad_lnM(b, q.A), s.v);
  } else {
    const QeExp e = qe_exp(mo);
    vn = qe_exp_next(e, U);
    if constexpr (MART) k0 = qe_k0_star(q, qe_exp_lnM(e, q.A), s.v);
  }
  s.x = qe_log_spot(q, s.x, s.v, vn, k0, zx);
  s.v = vn;
}

#if defined(__HIPCC__)
// Step k of a trajectory and (ANTI) its mirror on the draws of domain kDomQe under the trajectory's key (hh_qe.hip,
// hh_bates.hip): the normals of block (k, 0, 0, kDomQe); the mirror takes −Z_v, −Z_x and 1 − U.  The two branches
// diverge within a wave, and block (k, 1, 0, kDomQe) is drawn only by a lane one of whose members is in the exponential
// branch at step k — a branch, not a select over a block every lane would pay for.
template <bool ANTI, bool MART>
__device__ __forceinline__ void qe_pair_step(QeState& st, QeState& sa, const QeArgs& q, uint64_t key, uint32_t k) {
  double zv, zx;
  normal_pair(key, k, 0u, 0u, kDomQe, zv, zx);
  const QeMoments mo = qe_moments(q, st.v);
  const bool quad = mo.psi <= q.psi_c;
  QeMoments moa = mo;
  bool quada = true;
  if constexpr (ANTI) {
    moa = qe_moments(q, sa.v);
    quada = moa.psi <= q.psi_c;
  }
  double U = 0.5;  // read by a member in the exponential branch only
  if (!quad || !quada) {
    const Philox4 b = philox4x32_10(k, 1u, 0u, kDomQe, (uint32_t)key, (uint32_t)(key >> 32));
    U = u01_fast(b.c0, b.c1);
  }
  qe_member_step<MART>(st, q, mo, quad, zv, zx, U);
  if constexpr (ANTI) qe_member_step<MART>(sa, q, moa, quada, -zv, -zx, 1.0 - U);  // 1 − U is exact
}
#endif

}  // namespace hh
