"""A grid-PDE pricer: `CrankNicolsonMethod`, `PDESolution` and `solve(::PricingProblem{<:VanillaOption,
BlackScholesInputs}, ::CrankNicolsonMethod)`, with the grids on the device (`hh_fd_solve`, csrc/hh_fd.hip).  The
reference has no such method (its roadmap names a Crank–Nicolson solver); the scheme is stated in
include/hedgehog_mc.h and DESIGN §5.11.  A basket is one launch with one grid per payoff.

The host forms the per-option scalars (`fd_inputs`); the device steps the grid and returns the price with the
delta and gamma read off the three nodes round the spot.  A Dual input is refused, as in trees.py: the kernel
carries no partials — FiniteDifference works on the plain solves."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _ffi
from .dates import yearfrac
from .domain import (American, BlackScholesInputs, European, Forward, PricingProblem, Spot, VanillaOption, get_vol,
                     spine_zeros, zero_rate)
from .dual import n_partials
from .montecarlo import AbstractPricingMethod, MethodError


@dataclass(frozen=True)
class CrankNicolsonMethod(AbstractPricingMethod):
    """M = space_steps intervals in log-spot (even), N = time_steps, the first `rannacher` of them as two
    implicit-Euler half steps; the grid reaches n_std·σ√T + |ln(K/S0)| + |r − σ²/2|·T either side of ln S0."""
    space_steps: int
    time_steps: int
    n_std: float = 6.0
    rannacher: int = 2
    device: int = 0


@dataclass(frozen=True)
class PDESolution:
    problem: Any
    method: Any
    price: float
    delta: float
    gamma: float


def _style(payoff) -> int:
    if not isinstance(payoff, VanillaOption):
        raise MethodError("CrankNicolsonMethod prices a VanillaOption")
    if not isinstance(payoff.underlying, (Spot, Forward)):
        raise MethodError("CrankNicolsonMethod: Spot() or Forward() underlying")
    if isinstance(payoff.exercise_style, European):
        return _ffi.HH_FD_EUROPEAN   # the forward is the spot's at expiry: one European price for both
    if not isinstance(payoff.exercise_style, American):
        raise MethodError("CrankNicolsonMethod: European or American exercise")
    if isinstance(payoff.underlying, Forward):
        raise MethodError("CrankNicolsonMethod: an American option on Forward() is not a problem in the spot alone")
    return _ffi.HH_FD_AMERICAN


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _check(payoffs, m, method: CrankNicolsonMethod) -> None:
    M, N, R = method.space_steps, method.time_steps, method.rannacher
    if not (_is_int(M) and _is_int(N) and _is_int(R)):
        raise TypeError("CrankNicolsonMethod: space_steps, time_steps and rannacher must be integers")
    if M < 4 or M > _ffi.HH_FD_MAX_SPACE or M % 2:
        raise ValueError(f"CrankNicolsonMethod: space_steps = {M} is not an even number in 4 .. {_ffi.HH_FD_MAX_SPACE}")
    if N < 1 or N > _ffi.HH_FD_MAX_TIME:
        raise ValueError(f"CrankNicolsonMethod: time_steps = {N} outside 1 .. {_ffi.HH_FD_MAX_TIME}")
    if R < 0 or R > N:
        raise ValueError(f"CrankNicolsonMethod: rannacher = {R} outside 0 .. time_steps = {N}")
    if not (isinstance(method.n_std, (int, float)) and math.isfinite(method.n_std) and method.n_std > 0):
        raise ValueError(f"CrankNicolsonMethod: n_std = {method.n_std!r} must be a positive number")
    if not isinstance(m, BlackScholesInputs):
        raise MethodError(f"no method matching solve(PricingProblem{{VanillaOption, {type(m).__name__}}}, "
                          "CrankNicolsonMethod)")
    inputs = [m.spot, get_vol(m.sigma, None, None), *spine_zeros(m.rate)] + [p.strike for p in payoffs]
    if n_partials(*inputs) > 0:
        raise MethodError("ForwardAD through CrankNicolsonMethod is not carried (the grid kernel holds no partials); "
                          "use FiniteDifference")


@dataclass(frozen=True)
class FDInputs:
    """What hh_fd_solve receives for a list of payoffs on one market (fd_inputs)."""
    spots: np.ndarray
    strikes: np.ndarray
    cps: np.ndarray
    sigmas: np.ndarray
    rates: np.ndarray
    expiries: np.ndarray
    half_widths: np.ndarray
    styles: np.ndarray


def operator(sigma: float, r: float, h: float):
    """(lo, di, up) in the order of operations of csrc/hh_fd.h: fd_coef."""
    a = 0.5 * sigma * sigma
    b = r - a
    ah = a / (h * h)
    bh = b / (2.0 * h)
    return ah - bh, -2.0 * ah - r, ah + bh


def min_space_steps(sigma: float, r: float, W: float) -> int:
    """The smallest even M >= 4 with lo > 0 and up > 0: a/h² > |b|/(2h), h = 2W/M."""
    M = 4
    while M <= _ffi.HH_FD_MAX_SPACE:
        lo, _, up = operator(sigma, r, W / (M // 2))
        if lo > 0.0 and up > 0.0:
            return M
        M += 2
    return M


def fd_inputs(payoffs, market_inputs, method: CrankNicolsonMethod) -> FDInputs:
    """σ = get_vol(sigma, expiry, strike), r = zero_rate(rate, expiry), T = yearfrac(referenceDate, expiry),
    W = n_std·σ√T + |ln(K/S0)| + |r − σ²/2|·T.  Raises ValueError, naming the smallest M that would do, when the
    operator of an option is not positive off the diagonal."""
    m = market_inputs
    payoffs = list(payoffs)
    styles = [_style(p) for p in payoffs]
    _check(payoffs, m, method)
    n = len(payoffs)
    S, K, cp, sig, r, T, W = (np.empty(n) for _ in range(7))
    for k, p in enumerate(payoffs):
        S[k], K[k], cp[k] = float(m.spot), float(p.strike), p.call_put()
        sig[k] = float(get_vol(m.sigma, p.expiry, p.strike))
        r[k] = float(zero_rate(m.rate, p.expiry))
        T[k] = yearfrac(m.referenceDate, p.expiry)
        W[k] = method.n_std * sig[k] * math.sqrt(T[k]) + abs(math.log(K[k] / S[k])) + abs(r[k] - 0.5 * sig[k] * sig[k]) * T[k]
        lo, _, up = operator(sig[k], r[k], W[k] / (method.space_steps // 2))
        if not (lo > 0.0 and up > 0.0):
            need = min_space_steps(sig[k], r[k], W[k])
            hint = f"space_steps >= {need} is needed" if need <= _ffi.HH_FD_MAX_SPACE else \
                f"no space_steps up to {_ffi.HH_FD_MAX_SPACE} is enough"
            raise ValueError(f"CrankNicolsonMethod: payoff {k}: the grid is too coarse for its drift "
                             f"(lo = {lo!r}, up = {up!r}): {hint}")
    return FDInputs(S, K, cp, sig, r, T, W, np.array(styles, dtype=np.int32))


def fd_device(inp: FDInputs, space_steps: int, time_steps: int, rannacher: int, device: int = 0):
    """hh_fd_solve on prepared inputs: (prices, deltas, gammas), in order."""
    n = len(inp.spots)
    price, delta, gamma = np.empty(n), np.empty(n), np.empty(n)
    ctx = _ffi.get_context(device)
    ctx.check(ctx.lib.hh_fd_solve(ctx.handle, int(space_steps), int(time_steps), int(rannacher), n,
                                  inp.spots.ctypes.data, inp.strikes.ctypes.data, inp.cps.ctypes.data,
                                  inp.sigmas.ctypes.data, inp.rates.ctypes.data, inp.expiries.ctypes.data,
                                  inp.half_widths.ctypes.data, inp.styles.ctypes.data, price.ctypes.data,
                                  delta.ctypes.data, gamma.ctypes.data))
    return price, delta, gamma


def solve_pde_basket(payoffs, market_inputs, method: CrankNicolsonMethod) -> list:
    """solve(::BasketPricingProblem, ::CrankNicolsonMethod) — every grid in one launch; the solutions, in order.
    Each price equals (==) the payoff's own solve: the kernel form depends on space_steps alone."""
    payoffs = list(payoffs)
    if not payoffs:
        return []
    inp = fd_inputs(payoffs, market_inputs, method)
    price, delta, gamma = fd_device(inp, method.space_steps, method.time_steps, method.rannacher, method.device)
    return [PDESolution(PricingProblem(p, market_inputs), method, float(price[k]), float(delta[k]), float(gamma[k]))
            for k, p in enumerate(payoffs)]


def solve_pde(prob: PricingProblem, method: CrankNicolsonMethod) -> PDESolution:
    return solve_pde_basket([prob.payoff], prob.market_inputs, method)[0]
