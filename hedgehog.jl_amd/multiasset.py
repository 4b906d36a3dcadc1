"""Options on an index of several correlated lognormal assets (include/hedgehog_mc.h, "Several correlated lognormal
assets"; the reference prices one underlying only): baskets, spreads, geometric baskets, best-of and worst-of.

    inputs = MultiAssetInputs(reference_date, rate, spots, sigmas, correlation)
    option = IndexOption(WeightedSum((0.5, 0.3, 0.2)), VanillaOption(100.0, expiry, European(), Call(), Spot()))
    solve(PricingProblem(option, inputs), MonteCarlo(MultiAssetDynamics(), EulerMaruyama(), SimulationConfig(n, steps=…)))

The inner payoff — a European vanilla on the spot, an AsianOption, BarrierOption, DigitalOption or LookbackOption — is
read as written on the index.  One call of hh_mc_solve_path_assets simulates the assets and prices every payoff of one
index; in a BasketPricingProblem each distinct index takes one such pass, all on the same seeds.  The solves carry no dual
partials: Greeks come from FiniteDifference through AssetSpotLens, AssetVolLens and CorrelationLens (greeks.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any

from . import _ffi
from .dates import to_ticks, yearfrac
from .domain import (PATH_PAYOFFS, American, AsianOption, ContinuousMonitoring, European, FlatRateCurve, GeometricAverage, RateCurve,
                     Spot, VanillaOption, df, zero_rate)
from .dual import Dual, value_of
from .montecarlo import Antithetic, MethodError, MonteCarlo, path_monitoring, routes, run_paths

ROUTES = ("MonteCarlo(MultiAssetDynamics(), EulerMaruyama(), config) or MultiAssetAnalytic() on "
          "PricingProblem(IndexOption(index, payoff), MultiAssetInputs(…))")


class MultiAssetDynamics:
    """d correlated lognormal assets, d log S_i = (r − σ_i²/2) dt + σ_i dW_i, corr(dW_i, dW_j) = C_ij"""
    def __eq__(self, o): return type(o) is type(self)
    def __hash__(self): return hash("MultiAssetDynamics")
    def __repr__(self): return "MultiAssetDynamics()"


def _cholesky_ok(C):
    """the library's factorisation (csrc/hh_assets.h), for the one question it answers here: positive definite?"""
    d = len(C)
    L = [[0.0] * d for _ in range(d)]
    for i in range(d):
        for j in range(i + 1):
            s = C[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if j < i:
                L[i][j] = s / L[j][j]
            else:
                if not s > 0.0 or not math.isfinite(s):
                    return False
                L[i][i] = math.sqrt(s)
    return True


@dataclass(frozen=True)
class MultiAssetInputs:
    """The market of d = 1 … 8 assets under one rate curve: spots, flat volatilities and the d × d correlation matrix,
    validated here (ValueError): sizes, spots > 0, sigmas >= 0, a unit diagonal, symmetry, |C_ij| <= 1, positive
    definiteness by the library's own Cholesky factorisation."""
    referenceDate: int
    rate: Any
    spots: tuple
    sigmas: tuple
    correlation: tuple

    def __init__(self, reference_date, rate, spots, sigmas, correlation):
        ref = to_ticks(reference_date)
        if not isinstance(rate, (FlatRateCurve, RateCurve)):
            rate = FlatRateCurve(ref, rate)
        spots, sigmas = tuple(spots), tuple(sigmas)
        corr = tuple(tuple(row) for row in correlation)
        d = len(spots)
        if not 1 <= d <= _ffi.HH_MAX_ASSETS:
            raise ValueError(f"MultiAssetInputs: 1 … {_ffi.HH_MAX_ASSETS} assets, got {d}")
        if len(sigmas) != d or len(corr) != d or any(len(row) != d for row in corr):
            raise ValueError(f"MultiAssetInputs: {d} spots need {d} sigmas and a {d} × {d} correlation matrix")
        S, sg = [float(value_of(t)) for t in spots], [float(value_of(t)) for t in sigmas]
        Cm = [[float(value_of(t)) for t in row] for row in corr]
        if not all(math.isfinite(t) and t > 0.0 for t in S):
            raise ValueError("MultiAssetInputs: every spot must be finite and > 0")
        if not all(math.isfinite(t) and t >= 0.0 for t in sg):
            raise ValueError("MultiAssetInputs: every sigma must be finite and >= 0")
        if not all(math.isfinite(t) and abs(t) <= 1.0 for row in Cm for t in row):
            raise ValueError("MultiAssetInputs: every correlation must be finite and lie in [-1, 1]")
        if any(Cm[i][i] != 1.0 for i in range(d)):
            raise ValueError("MultiAssetInputs: the correlation matrix's diagonal must be 1")
        if any(Cm[i][j] != Cm[j][i] for i in range(d) for j in range(i)):
            raise ValueError("MultiAssetInputs: the correlation matrix must be symmetric")
        if not _cholesky_ok(Cm):
            raise ValueError("MultiAssetInputs: the correlation matrix is not positive definite")
        for k, v in (("referenceDate", ref), ("rate", rate), ("spots", spots), ("sigmas", sigmas), ("correlation", corr)):
            object.__setattr__(self, k, v)

    @property
    def n_assets(self):
        return len(self.spots)

    def replace(self, **kw):
        d = dict(reference_date=self.referenceDate, rate=self.rate, spots=self.spots, sigmas=self.sigmas,
                 correlation=self.correlation)
        d.update(kw)
        return MultiAssetInputs(**d)


# ---- the index -------------------------------------------------------------------------------------------------------------

def _weights(weights, what, positive=False, optional=False):
    if weights is None:
        if optional:
            return None
        raise ValueError(f"{what} needs weights")
    w = tuple(weights)
    if not 1 <= len(w) <= _ffi.HH_MAX_ASSETS:
        raise ValueError(f"{what}: 1 … {_ffi.HH_MAX_ASSETS} weights")
    v = [float(value_of(t)) for t in w]
    if not all(math.isfinite(t) for t in v):
        raise ValueError(f"{what}: every weight must be finite")
    if positive and not all(t > 0.0 for t in v):
        raise ValueError(f"{what}: every weight must be > 0")
    return w


@dataclass(frozen=True)
class WeightedSum:
    """Σ w_i S_i: an arithmetic basket; with weights of both signs a spread (which may be <= 0: a geometric Asian on it is
    refused)."""
    weights: tuple
    kind = _ffi.HH_INDEX_WEIGHTED_SUM

    def __post_init__(self):
        object.__setattr__(self, "weights", _weights(self.weights, "WeightedSum"))
        if not any(float(value_of(t)) != 0.0 for t in self.weights):
            raise ValueError("WeightedSum: every weight is zero")


@dataclass(frozen=True)
class GeometricMean:
    """Π S_i^{w_i}: lognormal, so a European vanilla on it has a closed form (MultiAssetAnalytic)"""
    weights: tuple
    kind = _ffi.HH_INDEX_GEOMETRIC

    def __post_init__(self):
        object.__setattr__(self, "weights", _weights(self.weights, "GeometricMean"))


@dataclass(frozen=True)
class BestOf:
    """max_i w_i S_i; weights=None: every weight is one"""
    weights: Any = None
    kind = _ffi.HH_INDEX_BEST_OF

    def __post_init__(self):
        object.__setattr__(self, "weights", _weights(self.weights, "BestOf", positive=True, optional=True))


@dataclass(frozen=True)
class WorstOf:
    """min_i w_i S_i; weights=None: every weight is one"""
    weights: Any = None
    kind = _ffi.HH_INDEX_WORST_OF

    def __post_init__(self):
        object.__setattr__(self, "weights", _weights(self.weights, "WorstOf", positive=True, optional=True))


INDEX_TYPES = (WeightedSum, GeometricMean, BestOf, WorstOf)
INNER_PAYOFFS = (VanillaOption,) + PATH_PAYOFFS


@dataclass(frozen=True)
class IndexOption:
    """`payoff` — a European VanillaOption on Spot, an AsianOption, BarrierOption, DigitalOption or LookbackOption — read as
    written on `index` in place of a spot"""
    index: Any
    payoff: Any

    def __post_init__(self):
        if not isinstance(self.index, INDEX_TYPES):
            raise TypeError("IndexOption.index must be a WeightedSum, GeometricMean, BestOf or WorstOf, got " + repr(self.index))
        if not isinstance(self.payoff, INNER_PAYOFFS):
            raise TypeError("IndexOption.payoff must be a VanillaOption, AsianOption, BarrierOption, DigitalOption or "
                            "LookbackOption, got " + repr(self.payoff))

    @property
    def expiry(self):
        return self.payoff.expiry


def is_multiasset(payoffs, market_inputs, method) -> bool:
    """Does anything of the triple name the multi-asset model?  Then only its routes may take it."""
    return isinstance(market_inputs, MultiAssetInputs) or isinstance(getattr(method, "dynamics", None), MultiAssetDynamics) or \
        any(isinstance(p, IndexOption) for p in payoffs)


def payoffs_of(prob):
    return list(prob.payoffs) if hasattr(prob, "payoffs") else [prob.payoff]


# ---- the route ----------------------------------------------------------------------------------------------------------------

def _require_route(payoffs, m, method):
    """every refusal that needs no device, or nothing; the words are the route's (routes.MULTIASSET)"""
    rt = routes()
    route = rt.MULTIASSET
    if not isinstance(method, MonteCarlo):
        raise MethodError(route.other_methods.format(type(method).__name__))
    rt.admitted(route, payoffs, m, method)
    for p in payoffs:
        if not isinstance(p, IndexOption):
            raise MethodError(f"a {type(p).__name__} names no index of the assets of MultiAssetInputs: wrap it in "
                              "IndexOption(index, payoff)")
        q = p.payoff
        if isinstance(getattr(q, "exercise_style", None), American):
            raise MethodError(route.no_american)
        if isinstance(q, VanillaOption) and not (isinstance(q.exercise_style, European) and isinstance(q.underlying, Spot)):
            raise MethodError("an IndexOption takes a European VanillaOption on Spot")
        if isinstance(getattr(q, "monitoring", None), ContinuousMonitoring):
            raise MethodError(route.no_continuous)
    if method.devices is not None:
        raise MethodError(route.one_device)
    flat = list(m.spots) + list(m.sigmas) + [t for row in m.correlation for t in row] + [zero_rate(m.rate, 0.0)]
    for p in payoffs:
        flat += list(p.index.weights or ())
    if any(isinstance(t, Dual) for t in flat):
        raise MethodError(route.no_duals)
    return route


def index_weights(index, d):
    w = (1.0,) * d if index.weights is None else index.weights
    if len(w) != d:
        raise ValueError(f"{type(index).__name__} has {len(w)} weights for {d} assets")
    return [float(t) for t in w]


def pack_assets(index, m: MultiAssetInputs) -> _ffi.hh_assets:
    return _ffi.make_assets([float(t) for t in m.spots], [float(t) for t in m.sigmas], index_weights(index, m.n_assets),
                            [[float(t) for t in row] for row in m.correlation], index.kind)


def index_groups(options, steps):
    """The passes of a set of IndexOptions: [(index, [positions])] in order of first appearance — options with an equal
    index, expiry and monitoring share one; one that reads the index at expiry alone rides along with the first pass of
    its index and expiry."""
    groups: dict = {}
    for i, o in enumerate(options):
        mon = path_monitoring(o.payoff, steps)
        if mon is not None:
            groups.setdefault((o.index, o.expiry, mon), []).append(i)
    for i, o in enumerate(options):
        if path_monitoring(o.payoff, steps) is None:
            key = next((k for k in groups if k[0] == o.index and k[1] == o.expiry), (o.index, o.expiry, None))
            groups.setdefault(key, []).append(i)
    return [(k, sorted(idx)) for k, idx in groups.items()]


def _solve_group(route, key, options, m, method, ensemble):
    """one pass: the options of one index that share an expiry and a monitoring.  The model carries the dates and the curve
    alone, the assets everything else: formed here, by hand."""
    index, expiry, mon = key
    cfg = method.config
    inner = [o.payoff for o in options]
    if index.kind == _ffi.HH_INDEX_WEIGHTED_SUM and any(w < 0.0 for w in index_weights(index, m.n_assets)) and \
            any(isinstance(q, AsianOption) and isinstance(q.averaging, GeometricAverage) for q in inner):
        raise MethodError("a geometric Asian on a WeightedSum with a negative weight: the index may be <= 0, where its "
                          "logarithm is not defined")
    model = _ffi.hh_model()
    model.T = float(yearfrac(m.referenceDate, expiry))
    model.r_drift = float(zero_rate(m.rate, 0.0))
    model.discount = float(df(m.rate, expiry))
    model.cp = 1.0
    c = _ffi.hh_config()
    c.dynamics, c.strategy, c.noise_mode = _ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, _ffi.HH_NOISE_GENERATE
    c.antithetic = int(isinstance(cfg.variance_reduction, Antithetic))
    c.n_steps, c.n_paths = cfg.steps, cfg.trajectories
    every, start = mon if mon is not None else (cfg.steps, False)
    return run_paths(route, options, m, method, ensemble, (model, c, every, start, (pack_assets(index, m),)), inner)


def solve_index_options(options, market_inputs, method, ensemble: bool = True):
    """IndexOptions on one market under one method: a MonteCarloSolution each, in order.  `ensemble`: the (5, n_total)
    statistics of the index (rows: enum hh_path_stat), shared by the solutions of a pass."""
    options = list(options)
    route = _require_route(options, market_inputs, method)
    for o in options:  # sizes, before any device is touched
        index_weights(o.index, market_inputs.n_assets)
    sols: list = [None] * len(options)
    for key, idx in index_groups(options, method.config.steps):
        for i, sol in zip(idx, _solve_group(route, key, [options[i] for i in idx], market_inputs, method, ensemble)):
            sols[i] = sol
    return sols
