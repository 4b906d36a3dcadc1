// The Crank–Nicolson scheme of hh_fd_solve (include/hedgehog_mc.h, "Crank–Nicolson finite differences") as functions
// the device kernels (hh_fd.hip), the host entry point and a host program share: the operator's coefficients, the
// constants of one (k, θ) phase, the maps a blocked scan composes, and one serial time step.  It includes nothing of
// HIP, so that tests/c/fd_host_check.cpp can price with it and run under the host sanitizers.  Internal; the public
// surface is include/hedgehog_mc.h.  DESIGN §5.11.
#pragma once
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

#if defined(__HIPCC__)
#define HH_FD_HD __host__ __device__
#else
#define HH_FD_HD
#endif

namespace hh {

// L V_j = lo·V_{j−1} + di·V_j + up·V_{j+1} on the uniform log-spot grid of spacing h
struct FdCoef {
  double lo, di, up;
};

HH_FD_HD inline FdCoef fd_coef(double sigma, double r, double h) {
  const double a = 0.5 * sigma * sigma;
  const double b = r - a;
  const double ah = a / (h * h);
  const double bh = b / (2.0 * h);
  FdCoef c;
  c.lo = ah - bh;
  c.di = -2.0 * ah - r;
  c.up = ah + bh;
  return c;
}

// what hh_fd_solve refuses: written so that a NaN fails it
HH_FD_HD inline bool fd_coef_ok(const FdCoef& c) { return c.lo > 0.0 && c.up > 0.0; }

// One phase (k, θ): row j of the step reads  −A·V_{j−1} + B·V_j − C·V_{j+1} = V_j + e·(lo·V_{j−1} + di·V_j + up·V_{j+1})
struct FdPhase {
  double A, B, C, e;
};

HH_FD_HD inline FdPhase fd_phase(const FdCoef& c, double k, double theta) {
  const double tk = theta * k;
  FdPhase p;
  p.A = tk * c.lo;
  p.B = 1.0 - tk * c.di;
  p.C = tk * c.up;
  p.e = (1.0 - theta) * k;
  return p;
}

HH_FD_HD inline double fd_rhs(const FdCoef& c, double e, double vm, double v, double vp) {
  return v + e * ((c.lo * vm + c.di * v) + c.up * vp);
}

HH_FD_HD inline double fd_max(double a, double b) { return a > b ? a : b; }

// x ↦ max(a·x + b, g), a >= 0: closed under composition.  g = −∞ (any value below every b) makes it affine.
struct FdMap {
  double a, b, g;
};

// second ∘ first
HH_FD_HD inline FdMap fd_compose(const FdMap& second, const FdMap& first) {
  FdMap m;
  m.a = second.a * first.a;
  m.b = second.a * first.b + second.b;
  m.g = fd_max(second.a * first.g + second.b, second.g);
  return m;
}

HH_FD_HD inline double fd_apply(const FdMap& m, double x) { return fd_max(m.a * x + m.b, m.g); }

// One serial time step on V[0 .. M] in place (Brennan–Schwartz when `american`): piv[M + 1] and y[M + 1] are
// work space, g[0 .. M] the payoff, v0_new / vM_new the Dirichlet ends at the new τ.  A put eliminates the
// super-diagonal from row M − 1 downwards and substitutes upwards from j = 1; a call mirrors it.
HH_FD_HD inline void fd_serial_step(double* V, const double* g, double* piv, double* y, int M, const FdCoef& c,
                                    const FdPhase& p, double cp, bool american, double v0_new, double vM_new) {
  for (int j = 1; j < M; ++j) y[j] = fd_rhs(c, p.e, V[j - 1], V[j], V[j + 1]);
  V[0] = v0_new;
  V[M] = vM_new;
  if (cp < 0.0) {
    y[M - 1] = y[M - 1] + p.C * V[M];
    piv[M - 1] = p.B;
    for (int j = M - 2; j >= 1; --j) {
      const double m = p.C / piv[j + 1];
      piv[j] = p.B - m * p.A;
      y[j] = y[j] + m * y[j + 1];
    }
    for (int j = 1; j < M; ++j) {
      const double x = (y[j] + p.A * V[j - 1]) / piv[j];
      V[j] = american ? fd_max(x, g[j]) : x;
    }
  } else {
    y[1] = y[1] + p.A * V[0];
    piv[1] = p.B;
    for (int j = 2; j < M; ++j) {
      const double m = p.A / piv[j - 1];
      piv[j] = p.B - m * p.C;
      y[j] = y[j] + m * y[j - 1];
    }
    for (int j = M - 1; j >= 1; --j) {
      const double x = (y[j] + p.C * V[j + 1]) / piv[j];
      V[j] = american ? fd_max(x, g[j]) : x;
    }
  }
}

}  // namespace hh
