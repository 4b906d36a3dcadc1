"""The two non-Monte-Carlo pricers the reference's MC tests and examples compare against, mirrored
so that such scripts run unchanged:

  BlackScholesAnalytic   /root/reference/src/pricing_methods/black_scholes.jl:38-64 — closed form,
                         evaluated on the host (a dozen flops; nothing to accelerate)
  CarrMadan(α, bound, dynamics)
                         /root/reference/src/pricing_methods/carr_madan.jl:15-92 — the Fourier
                         integral runs on the device (`hh_carr_madan`, csrc/hh_fourier.hip)
  MultiAssetAnalytic()   a European vanilla on a geometric index of several correlated lognormal assets, and Margrabe's
                         exchange option (the reference prices one underlying only): scalar code on the host
  VarianceGammaAnalytic() a European vanilla under the Variance Gamma model (the reference has none): the Black price
                         mixed over the gamma clock, a fixed trapezoidal rule on the host
  MertonAnalytic(n_terms) Merton's (1976) series for a European vanilla under jump diffusion (the reference has no
                         jump model): a Poisson-weighted sum of Black prices, scalar code on the host
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any

from . import _ffi
from .dates import yearfrac
from .domain import (BatesInputs, BlackScholesInputs, European, HestonInputs, MertonInputs, PricingProblem, VanillaOption,
                     VarianceGammaInputs, df, get_vol, zero_rate)
from .montecarlo import (BATES_ROUTES, VG_ROUTES, AbstractPricingMethod, BatesDynamics, HestonDynamics, LognormalDynamics,
                         MertonDynamics, MethodError, VarianceGammaDynamics, is_bates, is_vg)
from .multiasset import GeometricMean, IndexOption, MultiAssetInputs, WeightedSum, index_weights
from .domain import Spot


@dataclass(frozen=True)
class AnalyticSolution:
    """pricing_solutions.jl AnalyticSolution / CarrMadanSolution (price only)."""
    problem: Any
    method: Any
    price: float


class BlackScholesAnalytic(AbstractPricingMethod):
    def __eq__(self, o): return type(o) is type(self)
    def __hash__(self): return hash("BlackScholesAnalytic")


@dataclass(frozen=True)
class CarrMadan(AbstractPricingMethod):
    """carr_madan.jl:15-45: CarrMadan(α, bound, dynamics)."""
    α: float
    bound: float
    dynamics: Any
    compat_sqrt_alpha: bool = False   # montecarlo.jl:302 quirk Q1 for the lognormal law
    device: int = 0


def _ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def solve_black_scholes(prob: PricingProblem, method: BlackScholesAnalytic) -> AnalyticSolution:
    """black_scholes.jl:38-64."""
    payoff, m = prob.payoff, prob.market_inputs
    if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European)
            and isinstance(m, BlackScholesInputs)):
        raise MethodError("BlackScholesAnalytic: European VanillaOption on BlackScholesInputs")
    K = float(payoff.strike)
    sigma = float(get_vol(m.sigma, payoff.expiry, K))
    cp = payoff.call_put()
    T = yearfrac(m.referenceDate, payoff.expiry)
    D = float(df(m.rate, payoff.expiry))
    F = float(m.spot) / D
    if sigma == 0:
        price = D * max(cp * (F - K), 0.0)
    else:
        sq = math.sqrt(T)
        d1 = (math.log(F / K) + 0.5 * sigma * sigma * T) / (sigma * sq)
        d2 = d1 - sigma * sq
        price = D * cp * (F * _ncdf(cp * d1) - K * _ncdf(cp * d2))
    return AnalyticSolution(prob, method, price)


@dataclass(frozen=True)
class MertonAnalytic(AbstractPricingMethod):
    """Merton's series, truncated after n_terms Poisson weights (the weight of term n is e^{−λT}(λT)ⁿ/n!)."""
    n_terms: int = 200


def merton_series(S0, K, cp, sigma, lam, mu_j, sigma_j, T, D, n_terms=200, term=None):
    """Σ_n e^{−λT}(λT)ⁿ/n! · term(M_n, V_n): the jump count is Poisson(λT), and given n jumps log S_T is normal with
    mean M_n = log S0 − log D + (−σ²/2 − λκ̄)T + n·μ_J and variance V_n = σ²T + n·σ_J², κ̄ = exp(μ_J + σ_J²/2) − 1.
    term (default): the discounted Black price D·cp·(e^{M+V/2}·Φ(cp·d1) − K·Φ(cp·d2)), intrinsic where V = 0."""
    def black(M, V):
        F = math.exp(M + 0.5 * V)
        if V <= 0.0:
            return D * max(cp * (F - K), 0.0)
        sd = math.sqrt(V)
        d2 = (M - math.log(K)) / sd
        return D * cp * (F * _ncdf(cp * (d2 + sd)) - K * _ncdf(cp * d2))
    term = term or black
    kbar = math.expm1(mu_j + 0.5 * sigma_j * sigma_j)
    M0 = math.log(S0) - math.log(D) + (-0.5 * sigma * sigma - lam * kbar) * T
    w, total = math.exp(-lam * T), 0.0
    for n in range(int(n_terms)):
        if n:
            w = w * (lam * T) / n
        total += w * term(M0 + n * mu_j, sigma * sigma * T + n * sigma_j * sigma_j)
    return total


def solve_merton_analytic(prob: PricingProblem, method: MertonAnalytic) -> AnalyticSolution:
    payoff, m = prob.payoff, prob.market_inputs
    if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European)
            and isinstance(m, MertonInputs)):
        raise MethodError("MertonAnalytic: European VanillaOption on MertonInputs")
    T = yearfrac(m.referenceDate, payoff.expiry)
    price = merton_series(float(m.spot), float(payoff.strike), payoff.call_put(), float(get_vol(m.sigma, None, None)),
                          float(m.jump_intensity), float(m.jump_mean), float(m.jump_std), T,
                          float(df(m.rate, payoff.expiry)), method.n_terms)
    return AnalyticSolution(prob, method, price)


# ---- Variance Gamma (include/hedgehog_mc.h, "Variance Gamma") -------------------------------------------------------

@dataclass(frozen=True)
class VarianceGammaAnalytic(AbstractPricingMethod):
    """The gamma-mixing integral of a European vanilla: E_G[Black price given the clock G], G ~ Gamma(T/ν, ν)."""
    n_nodes: int = 4096


VG_MIX_CUT = 50.0  # the rule's nodes cover the clock's density down to e^-50 of its peak


def vg_mixing_price(S0, K, cp, sigma, theta, nu, T, r, D, n_nodes=4096):
    """D·E_G[cp·(F_G·Φ(cp·d1) − K·Φ(cp·d2))] with log F_G = log S0 + (r + ω)T + θG + σ²G/2 and log-variance σ²G over
    G ~ Gamma(a = T/ν, scale ν), ω = log(1 − θν − σ²ν/2)/ν.  The density's g^(a−1) singularity at 0 (a < 1) goes with the
    substitution g = ν·e^u: the weight becomes exp(a·u − e^u)/Γ(a), analytic on the whole line, decaying like e^{a·u} on
    the left and doubly exponentially on the right, and the trapezoidal rule converges geometrically in its step.  The
    rule is fixed: n_nodes equal steps between the two points where the weight has fallen to e^-50 of its peak at
    u = log a, so a sharply peaked clock (ν → 0) is resolved like a diffuse one."""
    arg = 1.0 - theta * nu - 0.5 * sigma * sigma * nu
    if not (nu > 0.0 and arg > 0.0):
        raise ValueError("Variance Gamma needs nu > 0 and 1 - theta nu - sigma^2 nu / 2 > 0")
    a = T / nu
    m0 = math.log(S0) + (r + math.log(arg) / nu) * T
    logK = math.log(K)
    phi = lambda u: a * u - math.exp(u)
    u0 = math.log(a)
    top = phi(u0)

    def edge(step):  # the point on that side of the mode where phi = top − VG_MIX_CUT, by doubling then bisection
        far = u0 + step
        while phi(far) > top - VG_MIX_CUT:
            step *= 2.0
            far = u0 + step
        near = u0
        for _ in range(200):
            mid = 0.5 * (near + far)
            if phi(mid) > top - VG_MIX_CUT:
                near = mid
            else:
                far = mid
        return far
    lo, hi = edge(-1.0), edge(1.0)
    n = int(n_nodes)
    h = (hi - lo) / n
    lg = math.lgamma(a)
    terms = []
    for i in range(n + 1):
        u = lo + i * h
        g = nu * math.exp(u)
        w = math.exp(phi(u) - lg) * (0.5 if i in (0, n) else 1.0)
        V = sigma * sigma * g
        M = m0 + theta * g
        if V <= 0.0:
            val = max(cp * (math.exp(M) - K), 0.0)
        else:
            sd = math.sqrt(V)
            d2 = (M - logK) / sd
            val = cp * (math.exp(M + 0.5 * V) * _ncdf(cp * (d2 + sd)) - K * _ncdf(cp * d2))
        terms.append(w * val)
    return D * math.fsum(terms) * h


def solve_vg_analytic(prob: PricingProblem, method: VarianceGammaAnalytic) -> AnalyticSolution:
    payoff, m = prob.payoff, prob.market_inputs
    if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European)
            and isinstance(m, VarianceGammaInputs)):
        raise MethodError("VarianceGammaAnalytic: European VanillaOption on VarianceGammaInputs")
    T = yearfrac(m.rate.reference_date, payoff.expiry)
    price = vg_mixing_price(float(m.spot), float(payoff.strike), payoff.call_put(), float(get_vol(m.sigma, None, None)),
                            float(m.theta), float(m.nu), T, float(zero_rate(m.rate, payoff.expiry)),
                            float(df(m.rate, payoff.expiry)), method.n_nodes)
    return AnalyticSolution(prob, method, price)


def _cm_payoff_arrays(payoffs, m, r_k, D_k, num=float):
    """The five arrays every Carr–Madan basket entry point takes — strikes, call/put signs, expiries, and the values
    (`num`) of the zero rates r_k and discount factors D_k of those expiries."""
    import numpy as np
    return (np.array([float(p.strike) for p in payoffs]), np.array([p.call_put() for p in payoffs], dtype=np.float64),
            np.array([yearfrac(m.rate.reference_date, p.expiry) for p in payoffs]),   # montecarlo.jl:301,317
            np.array([num(x) for x in r_k]), np.array([num(x) for x in D_k]))


# The laws beside the lognormal and Heston ones, in the order a problem is routed (first match of `routed`).  Per row: the
# guard of the dynamics / market-input pair and the MethodError text where it fails; the scalars scanned for Duals (no
# gradient form: a Dual anywhere is a MethodError, with the row's text) — first those of the hh_model fields named by
# `fields`, in that order, then the arguments of `struct`, the law's own C struct; the entry point.
_CM_LAWS = (
    dict(routed=is_bates,
         guard=lambda m, method: isinstance(method.dynamics, BatesDynamics) and isinstance(m, BatesInputs),
         guard_text=lambda m, method: (f"no Bates characteristic function for {type(method.dynamics).__name__} on "
                                       f"{type(m).__name__}: use {BATES_ROUTES}"),
         scalars=lambda m: [m.spot, m.V0, m.κ, m.θ, m.σ, m.ρ, m.jump_intensity, m.jump_mean, m.jump_std],
         fields=("S0", "V0", "kappa", "theta", "sigma", "rho"), struct=_ffi.make_jump, entry="hh_carr_madan_bates",
         dual_text="CarrMadan under BatesDynamics carries no dual partials (ForwardAD): use FiniteDifference"),
    dict(routed=is_vg,
         guard=lambda m, method: isinstance(method.dynamics, VarianceGammaDynamics) and isinstance(m, VarianceGammaInputs),
         guard_text=lambda m, method: (f"no Variance Gamma characteristic function for {type(method.dynamics).__name__} on "
                                       f"{type(m).__name__}: use {VG_ROUTES}"),
         scalars=lambda m: [m.spot, get_vol(m.sigma, None, None), m.theta, m.nu],
         fields=("S0", "sigma"), struct=_ffi.make_vg, entry="hh_carr_madan_vg",
         dual_text="CarrMadan under VarianceGammaDynamics carries no dual partials (ForwardAD): use FiniteDifference"),
    dict(routed=lambda m, method: isinstance(method.dynamics, MertonDynamics) or isinstance(m, MertonInputs),
         guard=lambda m, method: isinstance(method.dynamics, MertonDynamics) and isinstance(m, MertonInputs),
         guard_text=lambda m, method: "no marginal_law for this dynamics / market-input pair",
         scalars=lambda m: [m.spot, get_vol(m.sigma, None, None), m.jump_intensity, m.jump_mean, m.jump_std],
         fields=("S0", "sigma"), struct=_ffi.make_jump, entry="hh_carr_madan_jump",
         dual_text="CarrMadan under MertonDynamics carries no dual partials: use FiniteDifference"),
)


def _carr_madan_law(m, method: CarrMadan):
    """the row of _CM_LAWS a problem on these market inputs is routed to, or None: the lognormal and Heston laws"""
    for law in _CM_LAWS:  # a plain loop: this runs in front of every hh_carr_madan call, which takes 47 µs in all
        if law["routed"](m, method):
            return law
    return None


def _solve_carr_madan_law(payoffs, m, method: CarrMadan, law):
    """CarrMadan(α, bound, dynamics) under a law of _CM_LAWS: every payoff's integral in one launch of the law's entry
    point.  No gradient form: a Dual anywhere is a MethodError."""
    import numpy as np
    from .dual import Dual
    if not law["guard"](m, method):
        raise MethodError(law["guard_text"](m, method))
    scal = law["scalars"](m)
    r_k = [zero_rate(m.rate, p.expiry) for p in payoffs]
    D_k = [df(m.rate, p.expiry) for p in payoffs]
    if any(isinstance(v, Dual) for v in [*scal, *r_k, *D_k, *(p.strike for p in payoffs)]):
        raise MethodError(law["dual_text"])
    scal = [float(v) for v in scal]
    model, fields = _ffi.hh_model(), law["fields"]
    for name, v in zip(fields, scal):
        setattr(model, name, v)
    second = law["struct"](*scal[len(fields):])
    arrays = _cm_payoff_arrays(payoffs, m, r_k, D_k)
    out = np.empty(len(payoffs))
    ctx = _ffi.get_context(method.device)
    ctx.check(getattr(ctx.lib, law["entry"])(ctx.handle, C.byref(model), C.byref(second), float(method.α), float(method.bound),
                                             *[a.ctypes.data for a in arrays], len(payoffs), out.ctypes.data))
    return out


def _carr_madan_model(m, method: CarrMadan):
    """The model scalars every payoff on these market inputs shares (marginal_law, montecarlo.jl:293-320)
    -> (hh_model of their VALUES, dynamics, the scalars themselves — possibly Dual — in the order of
    enum hh_cm_grad: S0, V0, kappa, theta, sigma, rho)."""
    from .dual import value_of
    model = _ffi.hh_model()
    if isinstance(method.dynamics, HestonDynamics) and isinstance(m, HestonInputs):
        dyn = _ffi.HH_HESTON
        scal = [m.spot, m.V0, m.κ, m.θ, m.σ, m.ρ]
        model.V0, model.kappa, model.theta = value_of(m.V0), value_of(m.κ), value_of(m.θ)
        model.sigma, model.rho = value_of(m.σ), value_of(m.ρ)
    elif isinstance(method.dynamics, LognormalDynamics) and isinstance(m, BlackScholesInputs):
        dyn = _ffi.HH_LOGNORMAL
        vol = get_vol(m.sigma, None, None)
        scal = [m.spot, 0.0, 0.0, 0.0, vol, 0.0]
        model.sigma = value_of(vol)
    else:
        raise MethodError("no marginal_law for this dynamics / market-input pair")
    model.S0 = value_of(m.spot)
    return model, dyn, scal


def solve_carr_madan_basket(payoffs, market_inputs, method: CarrMadan):
    """solve(::BasketPricingProblem, ::CarrMadan) — basket.jl:35-38 over carr_madan.jl:47-71, the
    calibration objective's inner loop (calibration.jl:75-88): every payoff's Fourier integral in ONE
    launch (`hh_carr_madan_basket`, a workgroup per payoff).  Returns the prices in order."""
    import numpy as np
    m = market_inputs
    payoffs = list(payoffs)
    for payoff in payoffs:
        if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European)):
            raise MethodError("CarrMadan: European VanillaOption")
    from .dual import Dual, n_partials, partials_of, value_of
    law = _carr_madan_law(m, method)
    if law is not None:
        return _solve_carr_madan_law(payoffs, m, method, law)
    model, dyn, scal = _carr_madan_model(m, method)
    K = len(payoffs)
    if any(isinstance(p.strike, Dual) for p in payoffs):
        raise MethodError("CarrMadan basket: partials along a strike are not carried")
    r_k = [zero_rate(m.rate, p.expiry) for p in payoffs]                          # montecarlo.jl:299,318
    D_k = [df(m.rate, p.expiry) for p in payoffs]                                 # carr_madan.jl:89
    arrays = _cm_payoff_arrays(payoffs, m, r_k, D_k, value_of)
    out = np.empty(K)
    ctx = _ffi.get_context(method.device)
    args = (ctx.handle, C.byref(model), dyn, int(method.compat_sqrt_alpha), float(method.α),
            float(method.bound), *[a.ctypes.data for a in arrays], K, out.ctypes.data)
    P = n_partials(*scal, *r_k, *D_k)
    if P == 0:
        ctx.check(ctx.lib.hh_carr_madan_basket(*args))
        return out
    # a differentiated objective (calibration.jl:75-88 under AutoForwardDiff): the device returns the
    # gradient along the eight scalars of enum hh_cm_grad, the Dual prices are assembled here
    grad = np.empty((K, _ffi.HH_CM_GRAD_LEN))
    ctx.check(ctx.lib.hh_carr_madan_basket_grad(*args, grad.ctypes.data))
    seeds = np.array([partials_of(x, P) for x in scal])                # [6][P]
    prices = []
    for k in range(K):
        d = grad[k, :6] @ seeds + grad[k, 6] * np.array(partials_of(r_k[k], P)) \
            + grad[k, 7] * np.array(partials_of(D_k[k], P))
        prices.append(Dual(out[k], tuple(d)))
    return prices


def solve_carr_madan(prob: PricingProblem, method: CarrMadan) -> AnalyticSolution:
    """carr_madan.jl:47-71 with marginal_law (montecarlo.jl:293-320)."""
    payoff, m = prob.payoff, prob.market_inputs
    if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European)):
        raise MethodError("CarrMadan: European VanillaOption")
    from .dual import n_partials
    law = _carr_madan_law(m, method)
    if law is not None:  # a basket of one
        return AnalyticSolution(prob, method, float(_solve_carr_madan_law([payoff], m, method, law)[0]))
    model, dyn, scal = _carr_madan_model(m, method)
    r_k, D_k = zero_rate(m.rate, payoff.expiry), df(m.rate, payoff.expiry)
    if n_partials(*scal, r_k, D_k) > 0:
        # a Dual input (solve(GreekProblem(prob, lens), ForwardAD(), CarrMadan(...)), greeks_problem.jl:249-262):
        # the price must carry the partials — the gradient form, as a basket of one
        return AnalyticSolution(prob, method, solve_carr_madan_basket([payoff], m, method)[0])
    model.strike, model.cp = float(payoff.strike), payoff.call_put()
    model.T = yearfrac(m.rate.reference_date, payoff.expiry)      # montecarlo.jl:301,317
    model.r_drift = float(r_k)                                    # montecarlo.jl:299,318
    model.discount = float(D_k)                                   # carr_madan.jl:89
    out = C.c_double()
    ctx = _ffi.get_context(method.device)
    ctx.check(ctx.lib.hh_carr_madan(ctx.handle, C.byref(model), dyn, int(method.compat_sqrt_alpha),
                                    float(method.α), float(method.bound), C.byref(out)))
    return AnalyticSolution(prob, method, out.value)


# ---- several correlated lognormal assets (multiasset.py) ------------------------------------------------------------

@dataclass(frozen=True)
class MultiAssetAnalytic(AbstractPricingMethod):
    """The two closed forms that need no special function beyond Φ: a European vanilla on a GeometricMean index (which is
    lognormal), and Margrabe's exchange option — a call struck at 0 on WeightedSum((a, −b)), a, b > 0."""


def solve_multiasset_analytic(prob: PricingProblem, method: MultiAssetAnalytic):
    o, m = prob.payoff, prob.market_inputs
    q = getattr(o, "payoff", None)
    if not (isinstance(o, IndexOption) and isinstance(m, MultiAssetInputs) and isinstance(q, VanillaOption)
            and isinstance(q.exercise_style, European) and isinstance(q.underlying, Spot)):
        raise MethodError("MultiAssetAnalytic: an IndexOption of a European VanillaOption on MultiAssetInputs")
    d = m.n_assets
    w = index_weights(o.index, d)
    S, sg = [float(t) for t in m.spots], [float(t) for t in m.sigmas]
    Cm = [[float(t) for t in row] for row in m.correlation]
    T = float(yearfrac(m.referenceDate, q.expiry))
    r, D = float(zero_rate(m.rate, q.expiry)), float(df(m.rate, q.expiry))
    K, cp = float(q.strike), q.call_put()
    if isinstance(o.index, GeometricMean):
        mean = math.fsum(w[i] * (math.log(S[i]) + (r - 0.5 * sg[i] * sg[i]) * T) for i in range(d))
        var = T * math.fsum(w[i] * w[j] * sg[i] * sg[j] * Cm[i][j] for i in range(d) for j in range(d))
        if not K > 0.0:
            raise MethodError("MultiAssetAnalytic: a geometric-index vanilla needs a strike > 0")
        if var <= 0.0:
            price = D * max(cp * (math.exp(mean) - K), 0.0)
        else:
            sd = math.sqrt(var)
            d2 = (mean - math.log(K)) / sd
            price = D * cp * (math.exp(mean + 0.5 * var) * _ncdf(cp * (d2 + sd)) - K * _ncdf(cp * d2))
        return AnalyticSolution(prob, method, price)
    if isinstance(o.index, WeightedSum) and d == 2 and K == 0.0 and cp > 0.0 and w[0] > 0.0 and w[1] < 0.0:
        a, b = w[0] * S[0], -w[1] * S[1]
        var = (sg[0] * sg[0] + sg[1] * sg[1] - 2.0 * Cm[0][1] * sg[0] * sg[1]) * T
        if var <= 0.0:
            price = max(a - b, 0.0)
        else:
            sd = math.sqrt(var)
            d1 = (math.log(a / b) + 0.5 * var) / sd
            price = a * _ncdf(d1) - b * _ncdf(d1 - sd)
        return AnalyticSolution(prob, method, (D * math.exp(r * T)) * price)
    raise MethodError("MultiAssetAnalytic prices a European vanilla on a GeometricMean index and Margrabe's exchange option "
                      "(a call struck at 0 on WeightedSum((a, -b)) of two assets): use MonteCarlo(MultiAssetDynamics(), "
                      "EulerMaruyama(), config) for everything else")
