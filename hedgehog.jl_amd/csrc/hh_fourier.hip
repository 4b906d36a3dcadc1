// Carr–Madan Fourier price on the device: the analytic value the reference's
// Monte Carlo tests compare against (test/agreement/montecarlo_heston.jl:47-49, price_agreement.jl),
// so that a GPU box can self-check Heston / lognormal MC prices without a CPU-side quadrature.
//
// Reference: solve(prob, ::CarrMadan) src/pricing_methods/carr_madan.jl:47-71, call_transform
// :88-92, Heston log-price CF src/distributions/heston.jl:307-319, Normal-law CF
// src/distributions/sample_from_cf.jl:14-16, parity_transform src/payoffs/payoffs.jl:172-193.
// The reference integrates over (-bound, bound) with adaptive Gauss–Kronrod (QuadGK, third party);
// here 256 panels, one per lane, each cut into m equal sub-panels of 16-point Gauss–Legendre.
//
// The integrand is NOT entire: the damped transform has a pole at v = iα (the zero of α² + α − v² +
// iv(2α+1); the other one is at v = −i(α+1)), with residue ∝ ϕ(−i)·D = S0 whatever the model, strike and
// expiry.  A Gauss–Legendre panel of half-width h next to v = 0 therefore misses by about S0·f(h/α):
// rounding level (≤ 5e-14 at S0 = 100) for h/α ≤ 0.78, 2.4e-13 at 1.04, 6.2e-11 at 1.56, 4.5e-6 at 3.9
// (tests/test_carr_madan_exact_host.py pins these against the 40-digit integral).  So
//   m = carr_madan_subpanels(α, bound) = the smallest integer with bound/(256·m) ≤ 0.75·α,
// which is 1 — the plain 256-panel rule, bit for bit — for every setting the reference itself uses
// (α = 1, bound 16 and 32), and the entry points refuse bound/α > 192·kCarrMadanMaxSubpanels.
//
// Stated limit (not handled): for Heston the strip of analyticity of ϕ must contain Im u = −(α+1) for
// the expiry at hand; κ − ρσ(α+1) > 0 and (κ − ρσ(α+1))² ≥ σ²·α(α+1) make the (α+1)-th moment finite
// for every T.  Outside it the transform's own singularities approach the real line and no fixed rule
// converges; the kernels do not detect this.
//
// The unit is one rule (RuleArgs, carr_madan_kernel, carr_madan_grad_kernel) over one small type per law.  A law holds
// its own constants and has two members: set_payoff(T, r) forms what depends on a payoff's expiry and drift rate, cf(u)
// is the characteristic function of log S_T.  A further law is a further such type and a launcher of three lines.
#include <cmath>

#include "hh_kernels.h"

namespace hh {

namespace {

struct cz {
  double re, im;
};
__device__ __forceinline__ cz operator+(cz a, cz b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cz operator-(cz a, cz b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cz operator*(cz a, cz b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ cz operator*(double s, cz a) { return {s * a.re, s * a.im}; }
__device__ __forceinline__ cz zdiv(cz a, cz b) {
  const double inv = 1.0 / (b.re * b.re + b.im * b.im);
  return {(a.re * b.re + a.im * b.im) * inv, (a.im * b.re - a.re * b.im) * inv};
}
__device__ __forceinline__ cz zsqrt(cz z) {
  const double r = hypot(z.re, z.im);
  if (r == 0.0) return {0.0, 0.0};
  if (z.re >= 0.0) {
    const double t = sqrt(0.5 * (r + z.re));
    return {t, z.im / (2.0 * t)};
  }
  const double t = sqrt(0.5 * (r - z.re));
  return {fabs(z.im) / (2.0 * t), copysign(t, z.im)};
}
__device__ __forceinline__ cz zexp(cz z) {
  const double e = exp(z.re);
  double s, c;
  sincos(z.im, &s, &c);
  return {e * c, e * s};
}
__device__ __forceinline__ cz zlog(cz z) { return {log(hypot(z.re, z.im)), atan2(z.im, z.re)}; }

// ---- the rule and the payoffs ---------------------------------------------------------------------------------------------
struct RuleArgs {
  double alpha, bound;
  uint32_t m_sub;  // sub-panels per lane (carr_madan_subpanels)
  // basket form (one workgroup per payoff): per-payoff scalars in device memory, [4][n]: log K, T, r_drift, discount;
  // NULL = the one payoff of the scalars below, whose T and r the launcher has given to the law already
  const double* per_payoff;
  uint32_t n_payoffs;
  double* out;  // [blockIdx.x] = damped-call integral (the call price); the gradient form: [blockIdx.x][kGradVals]
  double logK, T, r, discount;
};

struct Payoff {
  double logK, T, r, discount;
};
__device__ __forceinline__ Payoff load_payoff(const RuleArgs& a, uint32_t k) {
  const uint32_t n = a.n_payoffs;
  return {a.per_payoff[k], a.per_payoff[n + k], a.per_payoff[2 * n + k], a.per_payoff[3 * n + k]};
}

// ---- the laws ---------------------------------------------------------------------------------------------------------------
// lognormal law (montecarlo.jl:293-303); sample_from_cf.jl:14-16: cf(Normal(μ, σ), t) = exp(i t μ − σ² t²/2)
struct NormalLaw {
  double logS0, sigma_ln;
  uint32_t compat_sqrt_alpha;
  double T, tmul, law_mu, law_sd;  // of the payoff
  __host__ __device__ void set_payoff(double T_, double r) {
    T = T_;
    const double sqT = sqrt(T);
    tmul = compat_sqrt_alpha ? sqT : T;
    law_mu = logS0 + (r - 0.5 * sigma_ln * sigma_ln) * tmul;  // montecarlo.jl:302
    law_sd = sigma_ln * sqT;
  }
  __device__ cz cf(cz t) const {
    const cz it = {-t.im, t.re};
    return zexp(law_mu * it - (0.5 * law_sd * law_sd) * (t * t));
  }
};

// Heston law (montecarlo.jl:310-320); heston.jl:307-319, complex argument u
struct HestonLaw {
  double logS0, V0, kappa, theta, sigma, rho;
  double T, r;  // of the payoff
  __host__ __device__ void set_payoff(double T_, double r_) { T = T_; r = r_; }
  __device__ __forceinline__ cz log_cf(cz u) const {
    const cz iu = {-u.im, u.re};
    const cz kri = {kappa - rho * sigma * iu.re, -rho * sigma * iu.im};  // κ − ρσ·iu
    const cz u2 = u * u;
    const cz d1 = zsqrt(kri * kri + (sigma * sigma) * (iu + u2));
    const cz g = zdiv(kri - d1, kri + d1);
    const cz ed = zexp({-d1.re * T, -d1.im * T});
    const cz one = {1.0, 0.0};
    const cz one_m_ged = one - g * ed;
    const cz C = (kappa * theta / (sigma * sigma)) * (T * (kri - d1) - 2.0 * zlog(zdiv(one_m_ged, one - g)));
    const cz Dv = (1.0 / (sigma * sigma)) * ((kri - d1) * zdiv(one - ed, one_m_ged));
    return C + V0 * Dv + logS0 * iu + (r * T) * iu;
  }
  __device__ cz cf(cz u) const { return zexp(log_cf(u)); }
};

// Merton (1976): log S_T = the lognormal law (law_mu carries the compensator −λκ̄T) + a compound Poisson sum of N(μ_J, σ_J²)
struct MertonLaw {
  NormalLaw n;
  double lam, mu_j, sigma_j, lam_kbar;
  __host__ __device__ void set_payoff(double T, double r) {
    n.set_payoff(T, r);
    // ((r − σ²/2) − λκ̄)·T, in that order: λ = 0 leaves the lognormal mean
    n.law_mu = n.logS0 + ((r - 0.5 * n.sigma_ln * n.sigma_ln) - lam_kbar) * T;
  }
  __device__ cz cf(cz t) const {
    const cz it = {-t.im, t.re};
    const cz t2 = t * t;
    const cz one = {1.0, 0.0};
    const cz jump = zexp(mu_j * it - (0.5 * sigma_j * sigma_j) * t2) - one;
    return zexp(n.law_mu * it - (0.5 * n.law_sd * n.law_sd) * t2 + (lam * n.T) * jump);
  }
};

// Bates (1996): the Heston law at r − λκ̄, the jump term (λ·T)·(exp(μ_J·iu − (½σ_J²)·u²) − 1) added to the exponent last
struct BatesLaw {
  HestonLaw h;
  double lam, mu_j, sigma_j, lam_kbar;
  __host__ __device__ void set_payoff(double T, double r) { h.set_payoff(T, r - lam_kbar); }  // λ = 0 leaves the Heston drift
  __device__ cz cf(cz u) const {
    const cz iu = {-u.im, u.re};
    const cz u2 = u * u;
    const cz one = {1.0, 0.0};
    cz e = h.log_cf(u);
    e = e + (lam * h.T) * (zexp(mu_j * iu - (0.5 * sigma_j * sigma_j) * u2) - one);
    return zexp(e);
  }
};

// Variance Gamma: exp(it·(log S0 + (r + ω)T)) · base^(−T/ν), base = 1 − θν·it + (σ²ν/2)·t², law_mu carrying the first
// factor's mean.  The power is exp(−(T/ν)·log base) with this unit's zlog, the principal branch: on the contour
// Im t = −(1+α) the real part of base is 1 − θν(1+α) + (σ²ν/2)(v² − (1+α)²) >= 1 − θν(1+α) − σ²ν(1+α)²/2, which the
// entry point has checked to be positive — base never crosses the negative real axis, so the branch is continuous
// along the whole contour.
struct VgLaw {
  double logS0;
  double theta_nu, half_s2nu, nu, omega;  // θ·ν, σ²ν/2, ν and the compensator ω (hh_vg.h: vg_omega), formed on the host
  double T, law_mu;                       // of the payoff
  __host__ __device__ void set_payoff(double T_, double r) {
    T = T_;
    law_mu = logS0 + (r + omega) * T;
  }
  __device__ cz cf(cz t) const {
    const cz it = {-t.im, t.re};
    const cz one = {1.0, 0.0};
    const cz base = one - theta_nu * it + half_s2nu * (t * t);
    return zexp(law_mu * it - (T / nu) * zlog(base));
  }
};

// carr_madan.jl:59-61, 88-92: damp · call_transform(v) · exp(−i v log K), real part
template <class Law>
__device__ double integrand(const Law& law, const RuleArgs& a, const Payoff& p, double v) {
  const cz u = {v, -(a.alpha + 1.0)};
  const cz phi = law.cf(u);
  const cz den = {a.alpha * a.alpha + a.alpha - v * v, v * (2.0 * a.alpha + 1.0)};
  const cz val = zdiv(p.discount * phi, den) * zexp({0.0, -v * p.logK});
  return exp(-a.alpha * p.logK) / 6.28318530717958647692 * val.re;
}

// ---- the rule's pieces ------------------------------------------------------------------------------------------------------
// 16-point Gauss–Legendre on [-1, 1] (positive half; symmetric)
__constant__ double kGLx[8] = {0.0950125098376374401853193, 0.2816035507792589132304605,
                               0.4580167776572273863424194, 0.6178762444026437484466718,
                               0.7554044083550030338951012, 0.8656312023878317438804679,
                               0.9445750230732325760779884, 0.9894009349916499325961542};
__constant__ double kGLw[8] = {0.1894506104550684962853967, 0.1826034150449235888667637,
                               0.1691565193950025381893121, 0.1495959888165767320815017,
                               0.1246289712555338720524763, 0.0951585116824927848099251,
                               0.0622535239386478928628438, 0.0271524594117540948517806};

// Centre of sub-panel j of this lane's panel (centre `mid`, m sub-panels of half-width hsub).  m = 1: the panel itself,
// with `mid` as the plain rule forms it, −bound + (lane + ½)·w — bit for bit.  m > 1: an exact integer times hsub.
// `mid` is rounded at the size of the bound, 1e-13 at bound 1000; next to v = 0, where the integrand is S0/(2πα) high and
// α wide, panels displaced by that much against each other cost (bound/α)·2e-17·S0 — 5e-12 at α = 0.1, bound 1000.
__device__ __forceinline__ double subpanel_centre(double mid, double hsub, uint32_t m, uint32_t j) {
  if (m == 1) return mid;
  return (double)(2 * (int)(threadIdx.x * m + j) + 1 - 256 * (int)m) * hsub;
}

// This lane's panel, sub-panel by sub-panel: body(centre, half-width)
template <class Body>
__device__ __forceinline__ void for_each_subpanel(const RuleArgs& a, Body body) {
  const double w = 2.0 * a.bound / 256.0;  // panel width
  const double mid = -a.bound + (threadIdx.x + 0.5) * w, half = 0.5 * w;
  const double hsub = half / (double)a.m_sub;
#pragma unroll 1
  for (uint32_t j = 0; j < a.m_sub; ++j) body(subpanel_centre(mid, hsub, a.m_sub, j), hsub);
}

// out[i] = the workgroup's sum of acc[i]: down each wave by shuffles, then the four waves in order
template <int N>
__device__ __forceinline__ void block_sum(const double (&acc)[N], double* out) {
  __shared__ double sm[4][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = acc[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < N)
    out[threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// The law and the payoff of this workgroup: payoff blockIdx.x of a basket with its expiry-dependent scalars, or the one
// payoff of the rule's own scalars
template <class Law>
__device__ __forceinline__ Payoff payoff_of_block(const RuleArgs& a, Law& law) {
  if (!a.per_payoff) return {a.logK, a.T, a.r, a.discount};
  const Payoff p = load_payoff(a, blockIdx.x);
  law.set_payoff(p.T, p.r);
  return p;
}

template <class Law>
__global__ __launch_bounds__(256) void carr_madan_kernel(const Law law0, const RuleArgs a) {
  Law law = law0;
  const Payoff p = payoff_of_block(a, law);
  double s[1] = {0.0};
  for_each_subpanel(a, [&](double msub, double hsub) {
    double sj = 0.0;
#pragma unroll 1
    for (int k = 0; k < 8; ++k)
      sj += kGLw[k] * (integrand(law, a, p, msub - hsub * kGLx[k]) + integrand(law, a, p, msub + hsub * kGLx[k]));
    s[0] += sj * hsub;
  });
  block_sum(s, a.out + blockIdx.x);
}

// ---- gradient of the price: complex numbers carrying P complex partials --------------------------
// The reference differentiates its calibration objective with ForwardDiff, i.e. pushes Duals through
// carr_madan.jl:47-92 and heston.jl:307-319.  Here the partials of the CF with respect to κ, σ, ρ are
// carried through the same expressions (3 directions); V0, θ, S0 and the rate enter log ϕ linearly:
//   log ϕ = C(κ,θ,σ,ρ) + V0·D(κ,σ,ρ) + iu (log S0 + rT),  C ∝ θ
//   ∂ϕ/∂V0 = ϕ D,  ∂ϕ/∂θ = ϕ C/θ,  ∂ϕ/∂S0 = ϕ iu/S0,  ∂ϕ/∂r = ϕ iu T.
template <int P>
struct zd {
  cz v;
  cz d[P];
};
template <int P>
__device__ __forceinline__ zd<P> operator+(const zd<P>& a, const zd<P>& b) {
  zd<P> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> operator-(const zd<P>& a, const zd<P>& b) {
  zd<P> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> operator*(const zd<P>& a, const zd<P>& b) {
  zd<P> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> operator*(cz s, const zd<P>& a) {
  zd<P> r;
  r.v = s * a.v;
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = s * a.d[k];
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> operator*(double s, const zd<P>& a) {
  return cz{s, 0.0} * a;
}
template <int P>
__device__ __forceinline__ zd<P> zdivd(const zd<P>& a, const zd<P>& b) {
  zd<P> r;
  const cz ib = zdiv({1.0, 0.0}, b.v);
  r.v = a.v * ib;
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * ib;
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> zsqrtd(const zd<P>& a) {
  zd<P> r;
  r.v = zsqrt(a.v);
  const cz h = zdiv({0.5, 0.0}, r.v);
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = a.d[k] * h;
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> zexpd(const zd<P>& a) {
  zd<P> r;
  r.v = zexp(a.v);
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = r.v * a.d[k];
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> zlogd(const zd<P>& a) {
  zd<P> r;
  r.v = zlog(a.v);
  const cz ia = zdiv({1.0, 0.0}, a.v);
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = a.d[k] * ia;
  return r;
}
template <int P>
__device__ __forceinline__ zd<P> zconst(double x, int dir = -1) {  // a real parameter, seeded along `dir`
  zd<P> r;
  r.v = {x, 0.0};
#pragma unroll
  for (int k = 0; k < P; ++k) r.d[k] = {k == dir ? 1.0 : 0.0, 0.0};
  return r;
}

// C and D of heston.jl:307-319 with their partials along (κ, σ, ρ); same expressions as HestonLaw::log_cf
__device__ void heston_CD(const HestonLaw& a, cz u, zd<3>& C, zd<3>& Dv) {
  const zd<3> kappa = zconst<3>(a.kappa, 0), sigma = zconst<3>(a.sigma, 1), rho = zconst<3>(a.rho, 2);
  const cz iu = {-u.im, u.re};
  const zd<3> rs = rho * sigma;
  const zd<3> kri = kappa - iu * rs;                              // κ − ρσ·iu
  const zd<3> s2 = sigma * sigma;
  const zd<3> d1 = zsqrtd(kri * kri + (iu + u * u) * s2);
  const zd<3> g = zdivd(kri - d1, kri + d1);
  const zd<3> ed = zexpd(cz{-a.T, 0.0} * d1);
  const zd<3> one = zconst<3>(1.0);
  const zd<3> one_m_ged = one - g * ed;
  const zd<3> kms = zdivd(kappa, s2);                             // κ/σ²  (· θ below)
  C = a.theta * (kms * (a.T * (kri - d1) - 2.0 * zlogd(zdivd(one_m_ged, one - g))));
  Dv = zdivd((kri - d1) * zdivd(one - ed, one_m_ged), s2);
}

// ϕ(u) and ∂ log ϕ along S0, V0, κ, θ, σ, ρ, r (dl comes in zeroed), law by law
__device__ __forceinline__ cz cf_with_partials(const HestonLaw& a, cz u, double S0, cz* dl) {
  const cz iu = {-u.im, u.re};
  zd<3> C, Dv;
  heston_CD(a, u, C, Dv);
  dl[0] = (1.0 / S0) * iu;
  dl[1] = Dv.v;
  dl[2] = C.d[0] + a.V0 * Dv.d[0];
  dl[3] = (1.0 / a.theta) * C.v;
  dl[4] = C.d[1] + a.V0 * Dv.d[1];
  dl[5] = C.d[2] + a.V0 * Dv.d[2];
  dl[6] = a.T * iu;
  return zexp(C.v + a.V0 * Dv.v + (a.logS0 + a.r * a.T) * iu);
}
// sample_from_cf.jl:14-16: log ϕ = i t μ − σ_T² t²/2, μ = log S0 + (r − σ²/2)·tmul
__device__ __forceinline__ cz cf_with_partials(const NormalLaw& a, cz t, double S0, cz* dl) {
  const cz it = {-t.im, t.re}, t2 = t * t;
  dl[0] = (1.0 / S0) * it;
  dl[4] = (-a.sigma_ln * a.tmul) * it - (a.sigma_ln * a.T) * t2;
  dl[6] = a.tmul * it;
  return zexp(a.law_mu * it - (0.5 * a.law_sd * a.law_sd) * t2);
}

// Price and gradient of one payoff per workgroup.  out[k][0] = call price, out[k][1..7] = its partials
// along S0, V0, κ, θ, σ, ρ, r_drift (lognormal: S0, σ, r_drift in slots 1, 5, 7; the others 0).
constexpr int kGradVals = 8;
template <class Law>
__global__ __launch_bounds__(256) void carr_madan_grad_kernel(const Law law0, const RuleArgs a) {
  Law law = law0;
  const Payoff p = payoff_of_block(a, law);
  const double S0 = exp(law.logS0);
  const double damp = exp(-a.alpha * p.logK) / 6.28318530717958647692;
  double acc[kGradVals];
#pragma unroll
  for (int i = 0; i < kGradVals; ++i) acc[i] = 0.0;
  auto node = [&](double v, double wt) {
    const cz u = {v, -(a.alpha + 1.0)};
    const cz den = {a.alpha * a.alpha + a.alpha - v * v, v * (2.0 * a.alpha + 1.0)};
    const cz kern = (wt * damp * p.discount) * (zdiv({1.0, 0.0}, den) * zexp({0.0, -v * p.logK}));
    cz dl[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) dl[i] = {0.0, 0.0};
    const cz phi = cf_with_partials(law, u, S0, dl);
    const cz base = kern * phi;
    acc[0] += base.re;
#pragma unroll
    for (int i = 0; i < 7; ++i) acc[1 + i] += (base * dl[i]).re;
  };
  for_each_subpanel(a, [&](double msub, double hsub) {
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      // the node below and the node above the centre, in that order, through ONE copy of the node's code: two copies
      // side by side are scheduled into each other and cost the Heston instance 100 more registers (408 against 304)
#pragma unroll 1
      for (int side = 0; side < 2; ++side)
        node(side ? msub + hsub * kGLx[k] : msub - hsub * kGLx[k], kGLw[k] * hsub);
    }
  });
  block_sum(acc, a.out + (size_t)blockIdx.x * kGradVals);
}

}  // namespace

uint32_t carr_madan_subpanels(double alpha, double bound) {
  const double m = ceil(bound / (256.0 * 0.75 * alpha));
  if (!(m <= (double)kCarrMadanMaxSubpanels)) return 0;
  return m < 1.0 ? 1u : (uint32_t)m;
}

// The rule of a launch: α, the bound and the sub-panels they ask for.  Refused where carr_madan_subpanels refuses: a
// rule of no sub-panels would write 0.0 as the price.
static int set_rule(RuleArgs& a, double alpha, double bound) {
  a.alpha = alpha; a.bound = bound;
  a.m_sub = carr_madan_subpanels(alpha, bound);
  return a.m_sub ? (int)hipSuccess : (int)hipErrorInvalidValue;
}

// One workgroup per payoff of `a` (one workgroup where it has no per_payoff) under `law`; GRAD: the gradient form
template <bool GRAD = false, class Law>
static int launch_rule(const Law& law, RuleArgs a, double alpha, double bound, hipStream_t s) {
  if (const int rc = set_rule(a, alpha, bound)) return rc;
  const dim3 grid(a.per_payoff ? a.n_payoffs : 1u);
  if constexpr (GRAD) hipLaunchKernelGGL(carr_madan_grad_kernel<Law>, grid, dim3(256), 0, s, law, a);
  else hipLaunchKernelGGL(carr_madan_kernel<Law>, grid, dim3(256), 0, s, law, a);
  return (int)hipGetLastError();
}

static RuleArgs basket_of(const double* per_payoff_dev, uint32_t n_payoffs, double* out_dev) {
  RuleArgs a{};
  a.per_payoff = per_payoff_dev;
  a.n_payoffs = n_payoffs;
  a.out = out_dev;
  return a;
}

static NormalLaw normal_law(const hh_model& m, int compat_sqrt_alpha) {
  NormalLaw l{};
  l.logS0 = log(m.S0);
  l.sigma_ln = m.sigma;
  l.compat_sqrt_alpha = (uint32_t)(compat_sqrt_alpha != 0);
  return l;
}

static HestonLaw heston_law(const hh_model& m) {
  HestonLaw l{};
  l.logS0 = log(m.S0); l.V0 = m.V0; l.kappa = m.kappa; l.theta = m.theta; l.sigma = m.sigma;
  l.rho = m.rho;
  return l;
}

int launch_carr_madan_basket(const hh_model& m, int dynamics, int compat_sqrt_alpha, double alpha,
                             double bound, const double* per_payoff_dev, uint32_t n_payoffs,
                             double* out_dev, hipStream_t s) {
  const RuleArgs a = basket_of(per_payoff_dev, n_payoffs, out_dev);
  if (dynamics == HH_HESTON) return launch_rule(heston_law(m), a, alpha, bound, s);
  return launch_rule(normal_law(m, compat_sqrt_alpha), a, alpha, bound, s);
}

int launch_carr_madan_grad(const hh_model& m, int dynamics, int compat_sqrt_alpha, double alpha,
                           double bound, const double* per_payoff_dev, uint32_t n_payoffs,
                           double* out_dev, hipStream_t s) {
  const RuleArgs a = basket_of(per_payoff_dev, n_payoffs, out_dev);
  if (dynamics == HH_HESTON) return launch_rule<true>(heston_law(m), a, alpha, bound, s);
  return launch_rule<true>(normal_law(m, compat_sqrt_alpha), a, alpha, bound, s);
}

int launch_carr_madan_jump(const hh_model& m, const hh_jump& jump, double alpha, double bound,
                           const double* per_payoff_dev, uint32_t n_payoffs, double* out_dev, hipStream_t s) {
  const MertonLaw law{normal_law(m, 0), jump.lambda, jump.mu_j, jump.sigma_j, merton_compensator(jump)};
  return launch_rule(law, basket_of(per_payoff_dev, n_payoffs, out_dev), alpha, bound, s);
}

int launch_carr_madan_bates(const hh_model& m, const hh_jump& jump, double alpha, double bound,
                            const double* per_payoff_dev, uint32_t n_payoffs, double* out_dev, hipStream_t s) {
  const BatesLaw law{heston_law(m), jump.lambda, jump.mu_j, jump.sigma_j, merton_compensator(jump)};
  return launch_rule(law, basket_of(per_payoff_dev, n_payoffs, out_dev), alpha, bound, s);
}

int launch_carr_madan_vg(const hh_model& m, const hh_vg& vg, double alpha, double bound, const double* per_payoff_dev,
                         uint32_t n_payoffs, double* out_dev, hipStream_t s) {
  VgLaw law{};
  law.logS0 = log(m.S0);
  law.theta_nu = vg.theta * vg.nu;
  law.half_s2nu = (0.5 * (m.sigma * m.sigma)) * vg.nu;
  law.nu = vg.nu;
  law.omega = vg_omega(m.sigma, vg);
  return launch_rule(law, basket_of(per_payoff_dev, n_payoffs, out_dev), alpha, bound, s);
}

// the single payoff of m: its scalars travel in the kernel's arguments, the law is given its T and r here
int launch_carr_madan(const hh_model& m, int dynamics, int compat_sqrt_alpha, double alpha,
                      double bound, double* out_dev, hipStream_t s) {
  RuleArgs a{};
  a.logK = log(m.strike); a.T = m.T; a.r = m.r_drift; a.discount = m.discount;
  a.out = out_dev;
  if (dynamics == HH_HESTON) {
    HestonLaw law = heston_law(m);
    law.set_payoff(m.T, m.r_drift);
    return launch_rule(law, a, alpha, bound, s);
  }
  NormalLaw law = normal_law(m, compat_sqrt_alpha);
  law.set_payoff(m.T, m.r_drift);
  return launch_rule(law, a, alpha, bound, s);
}

}  // namespace hh
