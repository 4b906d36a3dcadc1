"""Local volatility: dS = r·S·dt + σ(t, S)·S·dW on a tabulated surface σ(t, log S), and Dupire's formula to make one
(include/hedgehog_mc.h, "Local volatility on a tabulated surface"; the reference carries an interpolated RectVolSurface
in its market inputs and lists Dupire local vol on its roadmap — it has neither this model nor this route).

  LocalVolSurface(times, log_spots, vols)   σ at (times[j], log_spots[i]): linear interpolation, constant extrapolation;
                                            log_spots uniform (the device's grid is x_lo + i·h)
  get_local_vol(surf, t, S)                 the host evaluation of the device's lookup, operation for operation
  LocalVolInputs(referenceDate, rate, spot, surface), LocalVolDynamics()
  solve(PricingProblem | BasketPricingProblem, MonteCarlo(LocalVolDynamics(), EulerMaruyama(), config))
                                            European vanillas, Asians, barriers and lookbacks (also ContinuousMonitoring()),
                                            digitals: hh_mc_solve_path_lv, one simulation per (expiry, monitoring) group
  dupire_local_vol(call_price, …), dupire_from(market_inputs, method, …)
                                            σ² = 2(C_T + r·C_k)/(C_kk − C_k), k = log K, by central differences
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _ffi
from .dates import MILLISECONDS_IN_YEAR_365, to_ticks
from .domain import BlackScholesInputs, Call, European, FlatRateCurve, PricingProblem, RateCurve, Spot, VanillaOption
from .montecarlo import MethodError, MonteCarlo, PriceDynamics, routes, solve_path_payoffs

ROUTES = "MonteCarlo(LocalVolDynamics(), EulerMaruyama(), config) on LocalVolInputs"
UNIFORM_RTOL = 1e-12


class LocalVolDynamics(PriceDynamics): pass


@dataclass(frozen=True)
class LocalVolSurface:
    """σ at (times[j], log_spots[i]), vols[j][i]: times finite, >= 0 and strictly increasing, log_spots uniform (every
    spacing within 1e-12, relatively, of (last − first)/(n − 1)), every vol finite and > 0."""
    times: Any
    log_spots: Any
    vols: Any

    def __init__(self, times, log_spots, vols):
        t = np.array(times, dtype=np.float64).reshape(-1)
        x = np.array(log_spots, dtype=np.float64).reshape(-1)
        v = np.array(vols, dtype=np.float64)
        if t.size < 1 or x.size < 2 or v.shape != (t.size, x.size):
            raise ValueError("LocalVolSurface: times [n_times >= 1], log_spots [n_x >= 2], vols [n_times][n_x]")
        if t.size * x.size > _ffi.HH_LV_MAX_NODES:
            raise ValueError(f"LocalVolSurface: n_times * n_x = {t.size * x.size} is above HH_LV_MAX_NODES = {_ffi.HH_LV_MAX_NODES}")
        if not np.all(np.isfinite(t)) or np.any(t < 0.0) or np.any(np.diff(t) <= 0.0):
            raise ValueError("LocalVolSurface: times must be finite, >= 0 and strictly increasing")
        h = (x[-1] - x[0]) / (x.size - 1)
        if not np.all(np.isfinite(x)) or not h > 0.0 or np.any(np.abs(np.diff(x) - h) > UNIFORM_RTOL * h):
            raise ValueError("LocalVolSurface: log_spots must be finite, increasing and uniform (relative tolerance 1e-12): "
                             "non-uniform log-spot grids are not provided")
        if not np.all(np.isfinite(v)) or np.any(v <= 0.0):
            raise ValueError("LocalVolSurface: every vol must be finite and > 0")
        for a in (t, x, v):
            a.setflags(write=False)
        object.__setattr__(self, "times", t)
        object.__setattr__(self, "log_spots", x)
        object.__setattr__(self, "vols", v)

    x_lo = property(lambda s: float(s.log_spots[0]))
    h = property(lambda s: float((s.log_spots[-1] - s.log_spots[0]) / (s.log_spots.size - 1)))

    @classmethod
    def sample(cls, fn, times, x_lo, x_hi, n_x):
        """tabulate a callable σ(t, S) on times × exp(linspace(x_lo, x_hi, n_x))"""
        x = x_lo + (x_hi - x_lo) / (n_x - 1) * np.arange(n_x)
        return cls(times, x, [[float(fn(float(t), math.exp(xi))) for xi in x] for t in times])

    def c_struct(self) -> _ffi.hh_localvol:
        return _ffi.make_localvol(self.times, self.vols, self.x_lo, self.h)


def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def get_local_vol(surf: LocalVolSurface, t, S):
    """σ(t, S): the device's lookup (csrc/hh_localvol.h) on the host, one rounded operation each in its order — row and
    weight of t, cell of x = log S, time first, then x.  t plays t_k."""
    times, n_x = surf.times, surf.log_spots.size
    j, w = 0, 0.0
    if times.size > 1:
        while j + 2 < times.size and times[j + 1] <= t:
            j += 1
        w = min(max((float(t) - float(times[j])) / (float(times[j + 1]) - float(times[j])), 0.0), 1.0)
    u = (math.log(S) - surf.x_lo) * (1.0 / surf.h)
    u = min(max(u, 0.0), float(n_x - 1))
    i = min(int(u), n_x - 2)
    f = u - float(i)
    c0, c1 = float(surf.vols[j, i]), float(surf.vols[j, i + 1])
    if times.size > 1:
        c0 = _fma(w, float(surf.vols[j + 1, i]) - c0, c0)
        c1 = _fma(w, float(surf.vols[j + 1, i + 1]) - c1, c1)
    return _fma(f, c1 - c0, c0)


@dataclass(frozen=True)
class LocalVolInputs:
    """A spot, a rate curve and a local-volatility surface.  A class of its own, a subclass of no other inputs, so that
    no other model's route takes it silently."""
    referenceDate: int
    rate: Any
    spot: Any
    surface: LocalVolSurface

    def __init__(self, reference_date, rate, spot, surface):
        ref = to_ticks(reference_date)
        if not isinstance(rate, (FlatRateCurve, RateCurve)):
            rate = FlatRateCurve(ref, rate)
        if not isinstance(surface, LocalVolSurface):
            raise TypeError("LocalVolInputs: surface must be a LocalVolSurface")
        for k, v in (("referenceDate", ref), ("rate", rate), ("spot", spot), ("surface", surface)):
            object.__setattr__(self, k, v)

    def black_scholes(self, sigma=1.0):
        """the same spot and curve under a flat volatility (what the lognormal structs are formed on; the local-vol entry
        points do not read it)"""
        return BlackScholesInputs(self.referenceDate, self.rate, self.spot, sigma)


def is_localvol(market_inputs, method) -> bool:
    """Does anything of the pair name local volatility?  Then only its route may take it."""
    return isinstance(market_inputs, LocalVolInputs) or isinstance(getattr(method, "dynamics", None), LocalVolDynamics)


def refuse_other_methods(market_inputs, method):
    """CarrMadan, trees, PDE, LSM, analytic formulas on LocalVolInputs: a MethodError that names the route"""
    routes().LOCALVOL.refuse_method((), market_inputs, method)


def solve_localvol_payoffs(payoffs, market_inputs, method: MonteCarlo, ensemble: bool = True):
    """Payoffs that share an expiry, a monitoring and an extremes mode on ONE simulation (hh_mc_solve_path_lv): a
    MonteCarloSolution each, in order.  `ensemble`: the (5, n_total) statistics — (7, n_total) under
    ContinuousMonitoring() — shared by the solutions.  solve_path_payoffs held to this route: every other pair is refused."""
    return solve_path_payoffs(payoffs, market_inputs, method, ensemble, routes().LOCALVOL)


# ---- Dupire ------------------------------------------------------------------------------------------------------------

MIN_DENSITY = 1e-8  # a node is valid where C_kk − C_k > MIN_DENSITY · spot (and the numerator is > 0)


def dupire_local_vol(call_price, times, x_lo, x_hi, n_x, rate, dk, dT, vol_bounds=(0.01, 2.0), spot=None,
                     return_valid=False):
    """Dupire's local volatility on times × (x_lo + i·h), from any vectorised pricer call_price(T_array, K_array) of
    European calls under the flat rate `rate` (no dividends).  With k = log K and central differences of steps dk and
    dT around every node:  σ² = 2(C_T + r·C_k)/(C_kk − C_k).  A node is valid where the numerator and the denominator are
    positive and the denominator exceeds MIN_DENSITY·spot (C_kk − C_k = K²·C_KK: the density, which rounding swamps in
    the far wings); an invalid node takes its nearest valid neighbour in its row, towards the spot; everything is
    clamped to vol_bounds.  times[0] > dT (the lookup's constant extrapolation covers [0, times[0])).
    spot: the spot the prices are of (required).  return_valid: also the boolean array of valid nodes."""
    if spot is None or not spot > 0.0:
        raise ValueError("dupire_local_vol: spot (> 0) is required")
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    if not times[0] > dT:
        raise ValueError("dupire_local_vol: times[0] must be > dT (the stencil reaches times[0] − dT)")
    lo, hi = vol_bounds
    x = x_lo + (x_hi - x_lo) / (n_x - 1) * np.arange(n_x)
    T, X = np.meshgrid(times, x, indexing="ij")
    K = np.exp(X)
    up, dn = math.exp(dk), math.exp(-dk)
    stencil_T = np.stack([T, T, T, T + dT, T - dT])
    stencil_K = np.stack([K, K * up, K * dn, K, K])
    prices = np.asarray(call_price(stencil_T.reshape(-1), stencil_K.reshape(-1)), dtype=np.float64).reshape(stencil_T.shape)
    sig, valid = dupire_from_stencil(prices, rate, dk, dT, spot)
    i0 = int(np.argmin(np.abs(x - math.log(spot))))
    for j in range(times.size):
        if not valid[j, i0]:
            near = np.flatnonzero(valid[j])
            if near.size == 0:
                raise ValueError(f"dupire_local_vol: no valid node at time {times[j]}")
            sig[j, i0] = sig[j, near[np.argmin(np.abs(near - i0))]]
        for i in range(i0 + 1, n_x):
            if not valid[j, i]:
                sig[j, i] = sig[j, i - 1]
        for i in range(i0 - 1, -1, -1):
            if not valid[j, i]:
                sig[j, i] = sig[j, i + 1]
    surf = LocalVolSurface(times, x, np.clip(sig, lo, hi))
    return (surf, valid) if return_valid else surf


def dupire_from_stencil(prices, rate, dk, dT, spot):
    """prices [5][n_times][n_x]: C at (T, k), (T, k + dk), (T, k − dk), (T + dT, k), (T − dT, k) -> (σ, valid)"""
    C0, Cp, Cm, Cu, Cd = prices
    C_T = (Cu - Cd) / (2.0 * dT)
    C_k = (Cp - Cm) / (2.0 * dk)
    C_kk = (Cp - 2.0 * C0 + Cm) / (dk * dk)
    num, den = 2.0 * (C_T + rate * C_k), C_kk - C_k
    valid = (num > 0.0) & (den > MIN_DENSITY * spot)
    sig = np.sqrt(np.where(valid, num, 1.0) / np.where(valid, den, 1.0))
    return np.where(valid, sig, np.nan), valid


def dupire_from(market_inputs, method, times, x_lo, x_hi, n_x, dk, dT, vol_bounds=(0.01, 2.0)):
    """dupire_local_vol on the prices `method` gives under `market_inputs` — the device Carr–Madan (Heston, Merton,
    Bates) or BlackScholesAnalytic — every stencil point of the grid in ONE basket call.  The curve must be flat."""
    from .analytic import BlackScholesAnalytic, solve_black_scholes
    from .basket import BasketPricingProblem, solve_basket
    from .domain import zero_rate_yf
    ref = market_inputs.referenceDate
    if not isinstance(market_inputs.rate, FlatRateCurve):
        raise MethodError("dupire_from: a flat rate curve (Dupire's formula is written for a constant r here)")
    r = float(zero_rate_yf(market_inputs.rate, 1.0))

    def call_price(T, K):
        payoffs = [VanillaOption(float(k), ref + float(t) * MILLISECONDS_IN_YEAR_365, European(), Call(), Spot()) for t, k in zip(T, K)]
        if isinstance(method, BlackScholesAnalytic):
            return np.array([float(solve_black_scholes(PricingProblem(p, market_inputs), method).price) for p in payoffs])
        sols = solve_basket(BasketPricingProblem(payoffs, market_inputs), method).solutions
        return np.array([float(s.price) for s in sols])
    return dupire_local_vol(call_price, times, x_lo, x_hi, n_x, r, dk, dT, vol_bounds, spot=float(market_inputs.spot))
