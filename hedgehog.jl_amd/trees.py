"""Host mirror of /root/reference/src/pricing_methods/cox_ross_rubinstein.jl: `CoxRossRubinsteinMethod` (:23-25),
`CRRSolution` (src/solutions/pricing_solutions.jl:97-101) and `solve(::PricingProblem{<:VanillaOption},
::CoxRossRubinsteinMethod)` (:99-141), with the trees on the device (`hh_crr_solve`, csrc/hh_crr.hip).  A basket
(basket.jl:35-38) is one launch with one tree per payoff.

The host forms the per-tree scalars exactly as the reference writes them (`crr_inputs`); the device runs the
backward induction, bit for bit reproducible from those scalars.  A Dual input is refused: the
kernel carries no partials, and dropping them silently would return a wrong Greek — FiniteDifference works on
the plain solves."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _ffi
from .dates import MILLISECONDS_IN_YEAR_365, yearfrac
from .domain import (American, BlackScholesInputs, European, Forward, PricingProblem, Spot, VanillaOption, df,
                     get_vol, spine_zeros, zero_rate)
from .dual import n_partials
from .montecarlo import AbstractPricingMethod, MethodError


@dataclass(frozen=True)
class CoxRossRubinsteinMethod(AbstractPricingMethod):
    """cox_ross_rubinstein.jl:23-25: CoxRossRubinsteinMethod(steps); `device` picks the GPU."""
    steps: int
    device: int = 0


@dataclass(frozen=True)
class CRRSolution:
    """pricing_solutions.jl:97-101."""
    problem: Any
    method: Any
    price: float


def _style(payoff) -> int:
    if not isinstance(payoff, VanillaOption):
        raise MethodError("CoxRossRubinsteinMethod prices a VanillaOption")
    if isinstance(payoff.exercise_style, European):
        return _ffi.HH_CRR_EUROPEAN          # binomial_tree_value(…, ::European): the continuation alone
    if not isinstance(payoff.exercise_style, American):
        raise MethodError("CoxRossRubinsteinMethod: European or American exercise")
    if isinstance(payoff.underlying, Forward):
        return _ffi.HH_CRR_AMERICAN_FORWARD
    if isinstance(payoff.underlying, Spot):
        return _ffi.HH_CRR_AMERICAN_SPOT
    raise MethodError("CoxRossRubinsteinMethod: Spot() or Forward() underlying")


def _check(payoffs, m, steps: int) -> None:
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
        raise TypeError("CoxRossRubinsteinMethod.steps must be an integer")
    if steps < 1:
        raise ValueError(f"CoxRossRubinsteinMethod: steps = {steps} < 1 (the tree needs at least one step)")
    if steps > _ffi.HH_CRR_MAX_STEPS:
        raise ValueError(f"CoxRossRubinsteinMethod: steps = {steps} above HH_CRR_MAX_STEPS = {_ffi.HH_CRR_MAX_STEPS}")
    if not isinstance(m, BlackScholesInputs):
        # get_vol(market_inputs.sigma, …) exists for BlackScholesInputs only (HestonInputs: a MethodError there)
        raise MethodError(f"no method matching solve(PricingProblem{{VanillaOption, {type(m).__name__}}}, "
                          "CoxRossRubinsteinMethod)")
    inputs = [m.spot, get_vol(m.sigma, None, None), *spine_zeros(m.rate)] + [p.strike for p in payoffs]
    if n_partials(*inputs) > 0:
        raise MethodError("ForwardAD through CoxRossRubinsteinMethod is not carried (the tree kernel holds no "
                          "partials); use FiniteDifference")


def spot_factor_row(rate, steps: int, dT: float) -> np.ndarray:
    """binomial_tree_underlying(…, ::Spot) (cox_ross_rubinstein.jl:75-81) without the forward: element i is
    exp(−zero_rate(rate, add_yearfrac(rate.reference_date, i·ΔT))·(steps − i)·ΔT), in the reference's order
    of operations.  The reference date is integer ticks, so add_yearfrac(::Real, ::Real) keeps tᵢ a float."""
    row = np.empty(steps)
    for i in range(steps):
        t_i = rate.reference_date + (i * dT) * MILLISECONDS_IN_YEAR_365
        row[i] = math.exp(-float(zero_rate(rate, t_i)) * (steps - i) * dT)
    return row


@dataclass(frozen=True)
class CRRInputs:
    """What hh_crr_solve receives for a list of payoffs on one market (crr_inputs)."""
    forwards: np.ndarray
    strikes: np.ndarray
    cps: np.ndarray
    ups: np.ndarray
    discounts: np.ndarray
    styles: np.ndarray
    spot_factors: np.ndarray    # [n_rows, steps]
    spot_row_of_tree: np.ndarray


def crr_inputs(payoffs, market_inputs, steps: int) -> CRRInputs:
    """The reference's per-tree scalars (cox_ross_rubinstein.jl:107-124, 132): σ = get_vol(sigma, expiry,
    strike), T = yearfrac(referenceDate, expiry), F = spot / df(rate, expiry), ΔT = T / steps,
    u = exp(σ·√ΔT), per-step discount exp(−zero_rate(rate, expiry)·ΔT); the spot-factor rows of the
    Spot American payoffs, one per expiry."""
    m = market_inputs
    payoffs = list(payoffs)
    styles = [_style(p) for p in payoffs]
    _check(payoffs, m, steps)
    n = len(payoffs)
    F, K, cp, u, disc = (np.empty(n) for _ in range(5))
    rows: dict = {}
    row_of = np.zeros(n, dtype=np.uint32)
    for k, p in enumerate(payoffs):
        sigma = float(get_vol(m.sigma, p.expiry, p.strike))
        T = yearfrac(m.referenceDate, p.expiry)
        dT = T / steps
        F[k] = float(m.spot) / float(df(m.rate, p.expiry))
        K[k], cp[k] = float(p.strike), p.call_put()
        u[k] = math.exp(sigma * math.sqrt(dT))
        disc[k] = math.exp(-float(zero_rate(m.rate, p.expiry)) * dT)
        if styles[k] == _ffi.HH_CRR_AMERICAN_SPOT:
            if p.expiry not in rows:
                rows[p.expiry] = (len(rows), spot_factor_row(m.rate, steps, dT))
            row_of[k] = rows[p.expiry][0]
    sf = np.stack([r for _, r in rows.values()]) if rows else np.empty((0, steps))
    return CRRInputs(F, K, cp, u, disc, np.array(styles, dtype=np.int32), np.ascontiguousarray(sf), row_of)


def crr_device_prices(inp: CRRInputs, steps: int, device: int = 0) -> np.ndarray:
    """hh_crr_solve on prepared inputs: the prices, in order."""
    n = len(inp.forwards)
    out = np.empty(n)
    n_rows = inp.spot_factors.shape[0]
    ctx = _ffi.get_context(device)
    ctx.check(ctx.lib.hh_crr_solve(ctx.handle, int(steps), n, inp.forwards.ctypes.data, inp.strikes.ctypes.data,
                                   inp.cps.ctypes.data, inp.ups.ctypes.data, inp.discounts.ctypes.data,
                                   inp.styles.ctypes.data, inp.spot_factors.ctypes.data if n_rows else None,
                                   n_rows, inp.spot_row_of_tree.ctypes.data if n_rows else None, out.ctypes.data))
    return out


def solve_crr_basket(payoffs, market_inputs, method: CoxRossRubinsteinMethod) -> np.ndarray:
    """solve(::BasketPricingProblem, ::CoxRossRubinsteinMethod) — every tree in one launch; the prices, in order.
    Each equals (==) the payoff's own solve: the kernel form depends on the step count alone."""
    payoffs = list(payoffs)
    if not payoffs:
        return np.empty(0)
    return crr_device_prices(crr_inputs(payoffs, market_inputs, method.steps), method.steps, method.device)


def solve_crr(prob: PricingProblem, method: CoxRossRubinsteinMethod) -> CRRSolution:
    """cox_ross_rubinstein.jl:99-141 on the device."""
    price = solve_crr_basket([prob.payoff], prob.market_inputs, method)[0]
    return CRRSolution(prob, method, float(price))
