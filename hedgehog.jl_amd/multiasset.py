"""Options on an index of several correlated lognormal assets (include/hedgehog_mc.h, "Several correlated lognormal
assets"; the reference prices one underlying only): baskets, spreads, geometric baskets, best-of and worst-of.

    inputs = MultiAssetInputs(reference_date, rate, spots, sigmas, correlation)
    option = IndexOption(WeightedSum((0.5, 0.3, 0.2)), VanillaOption(100.0, expiry, European(), Call(), Spot()))
    solve(PricingProblem(option, inputs), MonteCarlo(MultiAssetDynamics(), EulerMaruyama(), SimulationConfig(n, steps=…)))

The inner payoff — a European vanilla on the spot, an AsianOption, BarrierOption, DigitalOption or LookbackOption — is
read as written on the index.  One call of hh_mc_solve_path_assets simulates the assets and prices every payoff of one
index; in a BasketPricingProblem each distinct index takes one such pass, all on the same seeds.  The solves carry no dual
partials: Greeks come from FiniteDifference through AssetSpotLens, AssetVolLens and CorrelationLens (greeks.py).

American and Bermudan exercise ("American exercise on several state rows"):
    option = IndexOption(WorstOf(), VanillaOption(100.0, expiry, American(), Put(), Spot()))
    solve(PricingProblem(option, inputs), LSM(MultiAssetDynamics(), EulerMaruyama(), config, degree), exercise_every=m)
regresses the continuation value on all monomials of the d standardised spots of total degree <= degree — C(d + degree,
degree) <= 45 functions — on every m-th step (hh_lsm_solve_assets).  simulate_asset_paths returns the rows.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import _ffi
from .dates import MILLISECONDS_IN_YEAR_365, to_ticks, yearfrac
from .domain import (PATH_PAYOFFS, American, AsianOption, ContinuousMonitoring, European, FlatRateCurve, GeometricAverage, RateCurve,
                     Spot, VanillaOption, df, zero_rate)
from .dual import Dual, value_of
from .montecarlo import Antithetic, MethodError, MonteCarlo, path_monitoring, routes, run_paths

ROUTES = ("MonteCarlo(MultiAssetDynamics(), EulerMaruyama(), config) or MultiAssetAnalytic() on "
          "PricingProblem(IndexOption(index, payoff), MultiAssetInputs(…))")
LSM_ROUTE = ("LSM(MultiAssetDynamics(), EulerMaruyama(), config, degree) on PricingProblem(IndexOption(index, VanillaOption(K, "
             "expiry, American(), cp, Spot())), MultiAssetInputs(…))")


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


# ---- American exercise: state rows and the several-variable induction ---------------------------------------------------------

def basis_count(d: int, degree: int) -> int:
    """C(d + degree, degree): the monomials of d variables of total degree <= degree"""
    return math.comb(d + degree, degree)


def _require_rows_route(prob, mc, exercise_every, american: bool):
    """every refusal of the state-row calls that needs no device, in the route's words; -> (route, index option, dates)"""
    rt = routes()
    route = rt.MULTIASSET
    option, m = prob.payoff, prob.market_inputs
    rt.admitted(route, [option], m, mc)
    if not isinstance(option, IndexOption):
        raise MethodError(f"a {type(option).__name__} names no index of the assets of MultiAssetInputs: wrap it in "
                          "IndexOption(index, payoff)")
    q = option.payoff
    if not isinstance(q, VanillaOption):
        raise MethodError(f"a path-dependent inner payoff ({type(q).__name__}) has no exercise decision to regress: " + LSM_ROUTE)
    if isinstance(getattr(q, "monitoring", None), ContinuousMonitoring):
        raise MethodError(route.no_continuous)
    if not isinstance(q.underlying, Spot) or (american and not isinstance(q.exercise_style, American)):
        raise MethodError("LSM on an index of several assets needs an American VanillaOption on Spot: " + LSM_ROUTE)
    if mc.devices is not None:
        raise MethodError(route.one_device)
    flat = list(m.spots) + list(m.sigmas) + [t for row in m.correlation for t in row] + [zero_rate(m.rate, 0.0), q.strike]
    flat += list(option.index.weights or ())
    if any(isinstance(t, Dual) for t in flat):
        raise MethodError(route.no_duals)
    every = int(exercise_every)
    steps = mc.config.steps
    if every != exercise_every or every < 1 or steps % every:
        raise MethodError(f"exercise_every ({exercise_every!r}) must be a whole number >= 1 that divides steps ({steps})")
    index_weights(option.index, m.n_assets)
    return route, option, steps // every


def _rows_structs(option, m, mc):
    """hh_model, hh_assets and hh_config of the walk to the option's expiry, on the seeds of mc.config in host memory"""
    cfg = mc.config
    q = option.payoff
    model = _ffi.hh_model()
    model.T = float(yearfrac(m.referenceDate, option.expiry))
    model.r_drift = float(zero_rate(m.rate, 0.0))
    model.discount = float(df(m.rate, option.expiry))
    model.strike, model.cp = float(q.strike), q.call_put()
    c = _ffi.hh_config()
    c.dynamics, c.strategy, c.noise_mode = _ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, _ffi.HH_NOISE_GENERATE
    c.antithetic = int(isinstance(cfg.variance_reduction, Antithetic))
    c.n_steps, c.n_paths = cfg.steps, cfg.trajectories
    c.seeds, c.seeds_on_device, c.seeds_len = cfg.seeds.ctypes.data, 0, cfg.seeds.size
    return model, pack_assets(option.index, m), c


@dataclass(frozen=True)
class AssetPaths:
    """The spots of the assets' trajectories on every exercise_every-th step: spot[date][asset][column], row j at times[j],
    date 0 the spots.  Antithetic: 2·trajectories columns, the mirror of trajectory i in column trajectories + i.  Under
    BestOf and WorstOf the rows are w_i·S_i — the weight is folded into the state the walk carries."""
    spot: Any
    times: Any
    result: Any = field(default=None, compare=False, repr=False)


def simulate_asset_paths(prob, mc, exercise_every=1) -> AssetPaths:
    """The assets' spots on the dates of solve(prob, LSM(mc, degree), exercise_every=…), on the same seeds, through
    hh_assets_path_rows: the device returns log-states, exp is taken here.  Under BestOf and WorstOf the rows are w_i·S_i.
    The inner payoff may be European or American: its expiry alone is read."""
    route, option, n_dates = _require_rows_route(prob, mc, exercise_every, american=False)
    model, assets, c = _rows_structs(option, prob.market_inputs, mc)
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    rows = np.empty((n_dates + 1, prob.market_inputs.n_assets, ntot))
    res = _ffi.hh_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_assets_path_rows(ctx.handle, C.byref(model), C.byref(assets), C.byref(c), int(exercise_every),
                                          rows.ctypes.data, 0, C.byref(res)))
    return AssetPaths(np.exp(rows), np.linspace(0.0, float(model.T), n_dates + 1), res)


def solve_index_lsm(prob, method, spot_paths: bool = False, stopping_info: bool = True, exercise_every=1):
    """An American (exercise_every > 1: Bermudan) IndexOption by Longstaff–Schwartz on the assets' state rows:
    hh_lsm_solve_assets.  stopping_info[0] counts exercise dates; spot_paths: AssetPaths.spot of the same trajectories."""
    from .lsm import LSMSolution
    mc = method.mc_method
    route, option, n_dates = _require_rows_route(prob, mc, exercise_every, american=True)
    m = prob.market_inputs
    B = basis_count(m.n_assets, method.degree)
    if not 1 <= method.degree <= 8 or B > _ffi.HH_LSM_MAX_BASIS:
        raise MethodError(f"LSM on {m.n_assets} assets at degree {method.degree} needs {B} basis functions: at most "
                          f"{_ffi.HH_LSM_MAX_BASIS}, degree 1 … 8 ({LSM_ROUTE})")
    model, assets, c = _rows_structs(option, m, mc)
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    tau = np.empty(ntot, dtype=np.int32) if stopping_info else None
    val = np.empty(ntot) if stopping_info else None
    rows = np.empty((n_dates + 1, m.n_assets, ntot)) if spot_paths else None
    date_discount = float(df(m.rate, m.referenceDate + (float(model.T) * int(exercise_every) / mc.config.steps) * MILLISECONDS_IN_YEAR_365))
    res = _ffi.hh_lsm_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_lsm_solve_assets(ctx.handle, C.byref(model), C.byref(assets), C.byref(c), int(exercise_every), method.degree,
                                          date_discount, C.byref(res), tau.ctypes.data if stopping_info else None,
                                          val.ctypes.data if stopping_info else None, rows.ctypes.data if spot_paths else None))
    return LSMSolution(prob, method, res.price, (tau, val) if stopping_info else None, np.exp(rows) if spot_paths else None,
                       std_error=res.std_error, result=res)
