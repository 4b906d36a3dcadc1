"""Host mirror of /root/reference/src/pricing_methods/least_squares_montecarlo.jl:
`LSM` (:12-34), `LSMSolution` (src/solutions/pricing_solutions.jl) and
`solve(::PricingProblem{VanillaOption{…,American,…}}, ::LSM)` (:99-136), running on the HIP path
(`hh_lsm_solve`).  Supported path sources: LognormalDynamics + BlackScholesExact, the pair the
reference's LSM is used with (test/agreement/american_options.jl), and HestonDynamics +
HestonBroadieKaya (per-date exact transitions, montecarlo.jl:209-231), regressed on the SPOT rows.
For every log-state problem (the Euler ones, and HestonNoise) the reference's extract_spot_grid
(:47-85) hands the regression log-prices.  The exact Heston paths are exponentiated first.  The Euler
combinations (LognormalDynamics or HestonDynamics + EulerMaruyama, `hh_lsm_solve_euler`) are reached
only when the caller names the path state: path_state="spot" regresses on exp(log S) as for the exact
Heston paths, path_state="log" hands log S to the regression and the payoff, the reference as run.
Without it they raise MethodError.

Every other spot-path model of routes.py — Merton jumps on Euler paths, HestonQE, Bates, local volatility, Variance Gamma —
is priced on the date rows of its own path kernel (`hh_lsm_solve_path`): LSM(dynamics, strategy, config, degree) with the
route's own dynamics, inputs and strategy.  `exercise_every=m` exercises on every m-th simulation step (a Bermudan
schedule of steps/m dates; m divides steps), there and on the Euler sources under path_state="spot".  Stopping times count
EXERCISE DATES, date j lying at T·j·m/steps, and spot_paths holds those dates' rows alone.

An American IndexOption on MultiAssetInputs under LSM(MultiAssetDynamics(), EulerMaruyama(), config, degree) is
multiasset.solve_index_lsm's: the assets' state rows and a regression on all monomials of the standardised spots up to
`degree` (`hh_lsm_solve_assets`); spot_paths is then the (dates + 1, assets, columns) array of simulate_asset_paths.

Under stochastic volatility the spot alone does not carry the continuation value.  regressors="spot_variance" regresses on
all monomials of the standardised spot AND variance up to `degree` (`hh_lsm_solve_path_states`: the walk's (log S, V) rows,
then the several-variable induction at m = 2) — on HestonDynamics + EulerMaruyama under path_state="spot", on HestonQE and
on Bates.  The default, regressors="spot", is every path above, unchanged.  simulate_state_paths returns the rows.

Each of these prices is in sample: the policy is valued on the trajectories it was fitted on.  fit_policy keeps the (S, V)
policy as an ExercisePolicy (`hh_lsm_fit_path_states`), policy_value runs it forward on other seeds — a lower bound
(`hh_lsm_policy_value_path`) — and upper_bound builds the Andersen–Broadie martingale from nested Heston Euler walks
(`hh_lsm_upper_bound`); solve(prob, DualBounds(LSM(...), outer=, inner=, fresh=, inner_seed=), exercise_every=m) does the three
and returns the bracket (BoundsSolution)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import _ffi
from .dates import MILLISECONDS_IN_YEAR_365, yearfrac
from .domain import (American, BlackScholesInputs, Call, European, HestonInputs, PricingProblem, Spot, VanillaOption, df,
                     get_vol, zero_rate)
from .dual import Dual
from .montecarlo import (AbstractPricingMethod, Antithetic, BlackScholesExact, EulerMaruyama,
                         HestonBroadieKaya, HestonDynamics, LognormalDynamics, MethodError, MonteCarlo, routes)

_PATH_STATES = {"spot": _ffi.HH_PATH_SPOT, "log": _ffi.HH_PATH_LOG}


@dataclass(frozen=True)
class LSM(AbstractPricingMethod):
    """least_squares_montecarlo.jl:12-34: LSM(mc_method, degree) or
    LSM(dynamics, strategy, config, degree)."""
    mc_method: MonteCarlo
    degree: int

    def __init__(self, *args):
        if len(args) == 2:
            mc, degree = args
        elif len(args) == 4:
            mc, degree = MonteCarlo(args[0], args[1], args[2]), args[3]
        else:
            raise TypeError("LSM(mc_method, degree) or LSM(dynamics, strategy, config, degree)")
        object.__setattr__(self, "mc_method", mc)
        object.__setattr__(self, "degree", int(degree))


@dataclass(frozen=True)
class LSMSolution:
    """pricing_solutions.jl LSMSolution: stopping_info = (times, values) arrays, spot_paths the
    (nsteps+1, npaths) matrix (None unless requested)."""
    problem: Any
    method: Any
    price: float
    stopping_info: Any
    spot_paths: Any
    std_error: float = field(default=float("nan"), compare=False)
    result: Any = field(default=None, compare=False, repr=False)


def _is_euler(mc: MonteCarlo) -> bool:
    return isinstance(mc.strategy, EulerMaruyama) and isinstance(mc.dynamics, (LognormalDynamics, HestonDynamics))


def _path_state_code(path_state) -> int:
    if path_state not in _PATH_STATES:
        raise ValueError(f'path_state must be "spot" or "log", not {path_state!r}')
    return _PATH_STATES[path_state]


def _lsm_structs(prob: PricingProblem, mc: MonteCarlo, euler: bool = False):
    """hh_model / hh_config of the path source behind an LSM solve (or a bare path simulation).
    euler: the Euler sources are admitted (the caller has named a path state)."""
    payoff, m = prob.payoff, prob.market_inputs
    cfg = mc.config
    from .dual import n_partials
    inputs = [getattr(m, a) for a in ("spot", "V0", "κ", "θ", "σ", "ρ") if hasattr(m, a)] + [payoff.strike]
    if isinstance(m, BlackScholesInputs):
        inputs.append(get_vol(m.sigma, None, None))
    if n_partials(*inputs, zero_rate(m.rate, 0.0)) > 0:
        # stopping decisions are not differentiable and the kernels carry no partials along full paths:
        # a Dual must not be dropped silently (float(Dual) would) — FiniteDifference works on plain solves
        raise MethodError("ForwardAD through the full-path kernels (LSM, exact Heston paths) is not carried; "
                          "use FiniteDifference")
    T = yearfrac(m.referenceDate, payoff.expiry)                       # :104, montecarlo.jl:147,219
    model = _ffi.hh_model()
    c = _ffi.hh_config()
    if isinstance(mc.dynamics, LognormalDynamics) and isinstance(mc.strategy, BlackScholesExact) \
            and isinstance(m, BlackScholesInputs):
        model.sigma = float(get_vol(m.sigma, None, None))
        c.dynamics, c.strategy = _ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW
    elif isinstance(mc.dynamics, HestonDynamics) and isinstance(mc.strategy, HestonBroadieKaya) \
            and isinstance(m, HestonInputs):
        model.V0, model.kappa, model.theta = float(m.V0), float(m.κ), float(m.θ)
        model.sigma, model.rho = float(m.σ), float(m.ρ)
        c.dynamics, c.strategy = _ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA
    elif euler and isinstance(mc.strategy, EulerMaruyama) and isinstance(mc.dynamics, LognormalDynamics) \
            and isinstance(m, BlackScholesInputs):
        model.sigma = float(get_vol(m.sigma, None, None))
        c.dynamics, c.strategy = _ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA
        c.em_split = int(mc.em_split)                                   # as montecarlo.py packs it
    elif euler and isinstance(mc.strategy, EulerMaruyama) and isinstance(mc.dynamics, HestonDynamics) \
            and isinstance(m, HestonInputs):
        model.V0, model.kappa, model.theta = float(m.V0), float(m.κ), float(m.θ)
        model.sigma, model.rho = float(m.σ), float(m.ρ)
        c.dynamics, c.strategy = _ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA
        c.em_split = int(mc.em_split)
    else:
        raise MethodError("full-path simulation on the HIP path: LognormalDynamics + BlackScholesExact "
                          "on BlackScholesInputs, or HestonDynamics + HestonBroadieKaya on HestonInputs")
    model.S0 = float(m.spot)
    model.r_drift = float(zero_rate(m.rate, 0.0))                      # montecarlo.jl:150,222
    model.T, model.strike, model.cp = float(T), float(payoff.strike), payoff.call_put()
    model.discount = 1.0
    c.antithetic = int(isinstance(cfg.variance_reduction, Antithetic))
    c.n_steps, c.n_paths = cfg.steps, cfg.trajectories
    c.seeds = cfg.seeds.ctypes.data
    c.seeds_len = cfg.seeds.size
    return model, c, T


def _exercise_dates(steps: int, exercise_every) -> int:
    every = int(exercise_every)
    if every != exercise_every or every < 1 or steps % every:
        raise MethodError(f"exercise_every ({exercise_every!r}) must be a whole number >= 1 that divides steps ({steps})")
    return steps // every


def _source_structs(prob: PricingProblem, mc: MonteCarlo, route, exercise_every):
    """(hh_path_source, hh_model, hh_config, T, n_dates) of the date rows of `route` (routes.py) for prob's payoff: the
    structs of the route's path solve to that expiry — formed by the route, with its refusals — under the payoff's strike and
    sign, on the seeds of mc.config in host memory."""
    payoff, m = prob.payoff, prob.market_inputs
    n_dates = _exercise_dates(mc.config.steps, exercise_every)
    model, c, extras = route.form_structs(VanillaOption(1.0, payoff.expiry, European(), Call(), Spot()), m, mc)
    if isinstance(payoff.strike, Dual):
        raise MethodError(route.no_duals)
    model.strike, model.cp = float(payoff.strike), payoff.call_put()
    c.seeds, c.seeds_on_device, c.seeds_len = mc.config.seeds.ctypes.data, 0, mc.config.seeds.size
    return routes().path_source(route, extras), model, c, float(model.T), n_dates


def _date_discount(m, T, steps, exercise_every) -> float:
    """df over one exercise period, T·exercise_every/steps from the reference date (:107 at exercise_every = 1)"""
    return float(df(m.rate, m.referenceDate + (T * exercise_every / steps) * MILLISECONDS_IN_YEAR_365))


def _solve_lsm_path(prob, method, source, model, c, T, n_dates, exercise_every, spot_paths, stopping_info) -> LSMSolution:
    """hh_lsm_solve_path: the grid of `source` on every exercise_every-th step, then the backward induction on it"""
    mc = method.mc_method
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    tau = np.empty(ntot, dtype=np.int32) if stopping_info else None
    val = np.empty(ntot) if stopping_info else None
    grid = np.empty((n_dates + 1, ntot)) if spot_paths else None
    res = _ffi.hh_lsm_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_lsm_solve_path(ctx.handle, C.byref(source), C.byref(model), C.byref(c), int(exercise_every),
                                        method.degree, _date_discount(prob.market_inputs, T, mc.config.steps, int(exercise_every)),
                                        C.byref(res), tau.ctypes.data if stopping_info else None,
                                        val.ctypes.data if stopping_info else None, grid.ctypes.data if spot_paths else None))
    return LSMSolution(prob, method, res.price, (tau, val) if stopping_info else None, grid, std_error=res.std_error, result=res)


_REGRESSORS = ("spot", "spot_variance")


def _state_structs(prob: PricingProblem, mc: MonteCarlo, exercise_every, path_state="spot"):
    """(hh_path_source, hh_model, hh_config, T, n_dates) of the (log S, V) rows of mc's walk: a spot-path route whose walk
    holds a variance (HestonQE, Bates) on its own triple, or HestonDynamics + EulerMaruyama; everything else is refused in
    the routes' words."""
    m = prob.market_inputs
    if routes().own_lsm_route_of(m, mc) is not None:
        raise MethodError("an index of several assets is regressed on its assets' spots: its walk has no variance; "
                          'regressors="spot_variance" needs ' + routes().STATE_ROWS)
    route = routes().lsm_route_of(m, mc)
    if route is not None and not route.state_rows:
        raise MethodError(f'the walk of {route.name} has no variance: regressors="spot_variance" needs ' + routes().STATE_ROWS)
    if path_state is not None and _path_state_code(path_state) == _ffi.HH_PATH_LOG:
        raise MethodError('regressors="spot_variance" regresses on the spot and the variance: path_state="log" is not offered with it')
    if route is not None:
        return _source_structs(prob, mc, route, exercise_every)
    if not (isinstance(mc.strategy, EulerMaruyama) and isinstance(mc.dynamics, HestonDynamics)):
        raise MethodError(f"the walk of {type(mc.dynamics).__name__} + {type(mc.strategy).__name__} has no variance rows: "
                          'regressors="spot_variance" needs ' + routes().STATE_ROWS)
    if path_state is None:
        raise MethodError('LSM on Euler paths needs a named path state: regressors="spot_variance" goes with path_state="spot"')
    if mc.devices is not None:
        raise MethodError("LSM on Euler paths is not sharded over several GPUs")
    n_dates = _exercise_dates(mc.config.steps, exercise_every)
    model, c, T = _lsm_structs(prob, mc, euler=True)
    return _ffi.make_path_source(routes().EULER.source), model, c, T, n_dates


def _states_of(rows: np.ndarray):
    """(spots, variances) of the device's rows[date][state][column]: exp is taken here, the variance is the walk's own"""
    return np.exp(rows[:, 0, :]), np.ascontiguousarray(rows[:, 1, :])


def _solve_lsm_states(prob, method, source, model, c, T, n_dates, exercise_every, spot_paths, stopping_info) -> LSMSolution:
    """hh_lsm_solve_path_states: the (log S, V) rows of `source` on every exercise_every-th step, then the several-variable
    induction on (S, V).  spot_paths: the (dates + 1, columns) spots, as the spot regression returns them."""
    mc = method.mc_method
    from .multiasset import basis_count  # C(2 + degree, degree) <= HH_LSM_MAX_BASIS
    if not 1 <= method.degree <= 8 or basis_count(2, method.degree) > _ffi.HH_LSM_MAX_BASIS:
        raise MethodError(f"LSM on (S, V) at degree {method.degree}: 1 <= degree <= 8 (C(2 + degree, degree) <= "
                          f"{_ffi.HH_LSM_MAX_BASIS} basis functions)")
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    tau = np.empty(ntot, dtype=np.int32) if stopping_info else None
    val = np.empty(ntot) if stopping_info else None
    rows = np.empty((n_dates + 1, 2, ntot)) if spot_paths else None
    res = _ffi.hh_lsm_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_lsm_solve_path_states(
        ctx.handle, C.byref(source), C.byref(model), C.byref(c), int(exercise_every), method.degree,
        _date_discount(prob.market_inputs, T, mc.config.steps, int(exercise_every)), C.byref(res),
        tau.ctypes.data if stopping_info else None, val.ctypes.data if stopping_info else None, None,
        rows.ctypes.data if spot_paths else None))
    return LSMSolution(prob, method, res.price, (tau, val) if stopping_info else None, _states_of(rows)[0] if spot_paths else None,
                       std_error=res.std_error, result=res)


def solve_lsm(prob: PricingProblem, method: LSM, spot_paths: bool = False,
              stopping_info: bool = True, path_state=None, exercise_every=1, regressors="spot") -> LSMSolution:
    """path_state: None (the exact sources only), "spot" or "log" (module docstring).  On an exact source
    "spot" is what it does anyway and "log" raises MethodError.  With path_state="log", spot_paths holds log S.
    exercise_every: exercise on every m-th step — on the spot-path models of routes.py, and (m > 1) on the Euler sources
    under path_state="spot"; stopping_info[0] then counts exercise dates, not steps, and spot_paths holds steps/m + 1 rows."""
    payoff, m = prob.payoff, prob.market_inputs
    mc = method.mc_method
    if regressors not in _REGRESSORS:
        raise ValueError(f'regressors must be "spot" or "spot_variance", not {regressors!r}')
    if regressors == "spot_variance":  # the walk's (log S, V) rows and the induction in two variables
        structs = _state_structs(prob, mc, exercise_every, path_state)
        if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, American)):
            raise MethodError("solve(::PricingProblem, ::LSM) needs an American VanillaOption")
        return _solve_lsm_states(prob, method, *structs, exercise_every, spot_paths, stopping_info)
    if routes().own_lsm_route_of(m, mc) is not None:  # several assets: an index, state rows and a basis in several variables
        from .multiasset import solve_index_lsm
        if path_state is not None:
            raise MethodError("path_state applies to the Euler path sources only: an index of several assets is regressed on "
                              "its assets' spots")
        return solve_index_lsm(prob, method, spot_paths, stopping_info, exercise_every)
    if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, American)):
        raise MethodError("solve(::PricingProblem, ::LSM) needs an American VanillaOption")
    state = None if path_state is None else _path_state_code(path_state)
    route = routes().lsm_route_of(m, mc)
    if route is not None:
        if state == _ffi.HH_PATH_LOG:
            raise MethodError('path_state="log" applies to the Euler path sources only')
        return _solve_lsm_path(prob, method, *_source_structs(prob, mc, route, exercise_every), exercise_every, spot_paths,
                               stopping_info)
    euler = state is not None and _is_euler(mc)
    if state == _ffi.HH_PATH_LOG and not euler:
        raise MethodError('path_state="log" applies to the Euler path sources only')
    model, c, T = _lsm_structs(prob, mc, euler=euler)
    cfg = mc.config
    nsteps = cfg.steps
    if exercise_every != 1:  # a Bermudan schedule: the Euler source's date rows
        n_dates = _exercise_dates(nsteps, exercise_every)
        if state == _ffi.HH_PATH_LOG:
            raise MethodError('exercise_every > 1 regresses on spot rows: path_state="log" exercises on every step')
        if not euler:
            raise MethodError('exercise_every > 1 needs path rows on a subset of the steps: the Euler sources under path_state="spot", '
                              "or a spot-path model (Merton, HestonQE, Bates, local volatility, Variance Gamma)")
        if mc.devices is not None:
            raise MethodError("LSM on Euler paths is not sharded over several GPUs")
        source = _ffi.make_path_source(routes().EULER.source)
        return _solve_lsm_path(prob, method, source, model, c, T, n_dates, exercise_every, spot_paths, stopping_info)
    # discount = df(rate, add_yearfrac(referenceDate, T / nsteps))      # :107
    step_discount = float(df(m.rate, m.referenceDate + (T / nsteps) * MILLISECONDS_IN_YEAR_365))
    ntot = cfg.trajectories * (2 if c.antithetic else 1)
    tau = np.empty(ntot, dtype=np.int32) if stopping_info else None
    val = np.empty(ntot) if stopping_info else None
    grid = np.empty((nsteps + 1, ntot)) if spot_paths else None
    res = _ffi.hh_lsm_result()
    if mc.devices is not None:  # ONE call, the trajectories sharded over these GPUs inside the library
        if euler:
            raise MethodError("LSM on Euler paths is not sharded over several GPUs")
        if spot_paths:
            raise ValueError("spot_paths is not returned by the multi-GPU form")
        mg = _ffi.get_multi_gpu(tuple(mc.devices))
        mg.check(mg.lib.hh_mgpu_lsm_solve(mg.handle, C.byref(model), C.byref(c), method.degree, step_discount,
                                          C.byref(res), tau.ctypes.data if stopping_info else None,
                                          val.ctypes.data if stopping_info else None))
        return LSMSolution(prob, method, res.price, (tau, val) if stopping_info else None, None,
                           std_error=res.std_error, result=res)
    ctx = _ffi.get_context(mc.device)
    outs = (tau.ctypes.data if stopping_info else None, val.ctypes.data if stopping_info else None,
            grid.ctypes.data if spot_paths else None)
    if euler:
        ctx.check(ctx.lib.hh_lsm_solve_euler(ctx.handle, C.byref(model), C.byref(c), state, method.degree,
                                             step_discount, C.byref(res), *outs))
    else:
        ctx.check(ctx.lib.hh_lsm_solve(ctx.handle, C.byref(model), C.byref(c), method.degree,
                                       step_discount, C.byref(res), *outs))
    return LSMSolution(prob, method, res.price, (tau, val) if stopping_info else None, grid,
                       std_error=res.std_error, result=res)


# ---- dual bounds: the policy as an object, its value on other seeds, the nested upper bound -------------------------------------

@dataclass(frozen=True)
class ExercisePolicy:
    """What an LSM fit decides by, free of the paths it was fitted on (hh_lsm_fit_path_states): `array` is the (dates + 1,
    2·m + B) matrix of the header's "Dual bounds for American exercise" — per date μ_i, isd_i of the m regressors, then the B
    coefficients; `discount` is the discount over one exercise period.  Any finite array of that shape is a policy.
    fit_seeds: the seeds the fit ran on (None for a hand-made policy); in_sample: the fit's LSMSolution."""
    array: Any
    m: int
    degree: int
    dates: int
    discount: float
    exercise_every: int = 1
    fit_seeds: Any = field(default=None, compare=False, repr=False)
    in_sample: Any = field(default=None, compare=False, repr=False)

    def __post_init__(self):
        from .multiasset import basis_count
        a = np.ascontiguousarray(self.array, dtype=np.float64)
        if a.shape != (self.dates + 1, 2 * self.m + basis_count(self.m, self.degree)):
            raise ValueError(f"a policy of {self.dates} dates, m = {self.m}, degree {self.degree} is a "
                             f"({self.dates + 1}, {2 * self.m + basis_count(self.m, self.degree)}) array, not {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError("a policy holds finite numbers only")
        object.__setattr__(self, "array", a)


@dataclass(frozen=True)
class DualBounds(AbstractPricingMethod):
    """solve(prob, DualBounds(LSM(...), outer=, inner=, fresh=, inner_seed=), exercise_every=m): the LSM policy fitted on the
    LSM config's seeds, valued on the `fresh` seeds (a lower bound) and bounded from above on the `outer` seeds with `inner`
    nested walks per date and outer column (Andersen–Broadie).  fresh, outer: seed arrays, or a count n — then the n seeds
    after the largest one used so far.  inner: a multiple of 64."""
    lsm: LSM
    outer: Any = 4096
    inner: int = 256
    fresh: Any = None
    inner_seed: int = 1

    def __init__(self, lsm, outer=4096, inner=256, fresh=None, inner_seed=1):
        for k, v in (("lsm", lsm), ("outer", outer), ("inner", int(inner)), ("fresh", fresh), ("inner_seed", int(inner_seed))):
            object.__setattr__(self, k, v)

    @property
    def mc_method(self):  # what routes.refuse_other_methods looks an LSM's walk up by
        return getattr(self.lsm, "mc_method", None)


@dataclass(frozen=True)
class BoundsSolution:
    """lower ± lower_se: the fitted policy on fresh paths; upper ± upper_se: the dual bound; in_sample: the LSM price on the
    fitted paths (neither bound); gap = upper − lower, gap_se = sqrt(upper_se² + lower_se²) — the seed sets are disjoint."""
    problem: Any
    method: Any
    lower: float
    lower_se: float
    upper: float
    upper_se: float
    in_sample: float
    in_sample_se: float
    gap: float
    gap_se: float
    policy: Any = field(default=None, compare=False, repr=False)
    result: Any = field(default=None, compare=False, repr=False)


def _american_vanilla(prob):
    if not (isinstance(prob.payoff, VanillaOption) and isinstance(prob.payoff.exercise_style, American)):
        raise MethodError("an exercise policy needs an American VanillaOption")


def _policy_degree(degree):
    from .multiasset import basis_count  # C(2 + degree, degree) <= HH_LSM_MAX_BASIS
    if not 1 <= degree <= 8 or basis_count(2, degree) > _ffi.HH_LSM_MAX_BASIS:
        raise MethodError(f"LSM on (S, V) at degree {degree}: 1 <= degree <= 8 (C(2 + degree, degree) <= "
                          f"{_ffi.HH_LSM_MAX_BASIS} basis functions)")


def _with_seeds(method: LSM, seeds) -> LSM:
    """`method` on other seeds: as many trajectories as seeds"""
    import dataclasses
    mc = method.mc_method
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    cfg = mc.config.replace(trajectories=int(seeds.size), seeds=seeds)
    return LSM(dataclasses.replace(mc, config=cfg), method.degree)


def _refuse_shared_seeds(what, seeds, fit_seeds):
    if fit_seeds is not None and np.intersect1d(np.asarray(seeds, dtype=np.uint64), np.asarray(fit_seeds, dtype=np.uint64)).size:
        raise MethodError(f"{what} seeds coincide with the seeds the policy was fitted on: the value of a policy on its own paths "
                          "is no lower bound (look-ahead bias) — hand in other seeds")


def fit_policy(prob: PricingProblem, method: LSM, exercise_every=1, regressors="spot_variance", path_state="spot") -> ExercisePolicy:
    """The LSM induction of solve(prob, method, regressors="spot_variance", …) with its policy kept (hh_lsm_fit_path_states):
    HestonDynamics + EulerMaruyama, HestonQE and Bates."""
    if regressors != "spot_variance":
        raise MethodError('fit_policy keeps the policy of the regression on (S, V): regressors="spot_variance" (the one-variable '
                          "inductions keep none)")
    mc = method.mc_method
    source, model, c, T, n_dates = _state_structs(prob, mc, exercise_every, path_state)
    _american_vanilla(prob)
    _policy_degree(method.degree)
    D = _date_discount(prob.market_inputs, T, mc.config.steps, int(exercise_every))
    from .multiasset import basis_count
    array = np.empty((n_dates + 1, 4 + basis_count(2, method.degree)))
    res = _ffi.hh_lsm_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_lsm_fit_path_states(ctx.handle, C.byref(source), C.byref(model), C.byref(c), int(exercise_every),
                                             method.degree, D, C.byref(res), array.ctypes.data))
    sol = LSMSolution(prob, method, res.price, None, None, std_error=res.std_error, result=res)
    return ExercisePolicy(array, 2, method.degree, n_dates, D, int(exercise_every), np.array(mc.config.seeds, dtype=np.uint64), sol)


def _check_policy_fits(policy: ExercisePolicy, method: LSM, n_dates, exercise_every, D):
    if not isinstance(policy, ExercisePolicy):
        raise TypeError("policy must be an ExercisePolicy")
    if policy.m != 2:
        raise MethodError(f"a policy in {policy.m} regressors does not decide on (S, V) rows: m = 2")
    if (policy.dates, policy.degree) != (n_dates, method.degree):
        raise MethodError(f"the policy has {policy.dates} dates at degree {policy.degree}; the method asks for {n_dates} dates "
                          f"(steps / exercise_every) at degree {method.degree}")
    if abs(policy.discount - D) > 1e-12 * D:
        raise MethodError(f"the policy discounts an exercise period by {policy.discount!r}, the problem by {D!r}")


def policy_value(prob: PricingProblem, method: LSM, policy: ExercisePolicy, seeds=None, exercise_every=None,
                 path_state="spot") -> LSMSolution:
    """The policy run forward on the walk of `method` on `seeds` (default: the method's own) through hh_lsm_policy_value_path:
    with seeds other than the fit's, an out-of-sample LOWER bound.  Seeds the policy was fitted on are refused."""
    every = policy.exercise_every if exercise_every is None and isinstance(policy, ExercisePolicy) else (exercise_every or 1)
    if seeds is not None:
        method = _with_seeds(method, seeds)
    mc = method.mc_method
    source, model, c, T, n_dates = _state_structs(prob, mc, every, path_state)
    _american_vanilla(prob)
    _policy_degree(method.degree)
    D = _date_discount(prob.market_inputs, T, mc.config.steps, int(every))
    _check_policy_fits(policy, method, n_dates, every, D)
    _refuse_shared_seeds("policy_value:", mc.config.seeds[:mc.config.trajectories], policy.fit_seeds)
    res = _ffi.hh_lsm_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_lsm_policy_value_path(ctx.handle, C.byref(source), C.byref(model), C.byref(c), int(every),
                                               policy.array.ctypes.data, method.degree, D, C.byref(res)))
    return LSMSolution(prob, method, res.price, None, None, std_error=res.std_error, result=res)


def upper_bound(prob: PricingProblem, method: LSM, policy: ExercisePolicy, outer, inner=256, inner_seed=1, exercise_every=None,
                want_cont=False):
    """The dual upper bound of `policy` on the outer seeds (hh_lsm_upper_bound): HestonDynamics + EulerMaruyama, plain paths.
    Returns the hh_bounds_result, and with want_cont (cont, cont_se, pathwise_max) beside it."""
    every = policy.exercise_every if exercise_every is None and isinstance(policy, ExercisePolicy) else (exercise_every or 1)
    routes().bounds_route_of(prob.market_inputs, method.mc_method)
    method = _with_seeds(method, outer)
    mc = method.mc_method
    if isinstance(mc.config.variance_reduction, Antithetic):
        raise MethodError("DualBounds: antithetic outer paths are not offered (the martingale is built per outer column): use "
                          "NoVarianceReduction()")
    if int(inner) <= 0 or int(inner) % 64:
        raise MethodError(f"DualBounds: inner ({inner}) must be a multiple of 64 and >= 64")
    source, model, c, T, n_dates = _state_structs(prob, mc, every, "spot")
    _american_vanilla(prob)
    _policy_degree(method.degree)
    D = _date_discount(prob.market_inputs, T, mc.config.steps, int(every))
    _check_policy_fits(policy, method, n_dates, every, D)
    n = mc.config.trajectories
    cont = np.empty((n_dates, n)) if want_cont else None
    cont_se = np.empty((n_dates, n)) if want_cont else None
    pmax = np.empty(n) if want_cont else None
    res = _ffi.hh_bounds_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_lsm_upper_bound(ctx.handle, C.byref(model), C.byref(c), int(every), policy.array.ctypes.data,
                                         method.degree, D, int(inner), int(inner_seed) & (2**64 - 1), C.byref(res),
                                         cont.ctypes.data if want_cont else None, cont_se.ctypes.data if want_cont else None,
                                         pmax.ctypes.data if want_cont else None))
    return (res, cont, cont_se, pmax) if want_cont else res


def _seed_set(spec, used_max, what):
    """a seed array as given, or the `spec` seeds after used_max"""
    if spec is None:
        raise MethodError(f"DualBounds needs {what}: a seed array, or a count")
    if np.ndim(spec) == 0:
        n = int(spec)
        if n < 1:
            raise MethodError(f"DualBounds: {what} must hold at least one seed")
        return np.arange(used_max + 1, used_max + 1 + n, dtype=np.uint64)
    return np.ascontiguousarray(spec, dtype=np.uint64)


def solve_dual_bounds(prob: PricingProblem, method: DualBounds, exercise_every=1, path_state="spot") -> BoundsSolution:
    """fit on the LSM config's seeds, value on `fresh`, bound on `outer` (module docstring of DualBounds)"""
    lsm = method.lsm
    if not isinstance(lsm, LSM):
        raise MethodError("DualBounds(LSM(...), outer=, inner=, fresh=, inner_seed=)")
    routes().bounds_route_of(prob.market_inputs, lsm.mc_method)  # a route that cannot serve says so before anything runs
    if isinstance(lsm.mc_method.config.variance_reduction, Antithetic):
        raise MethodError("DualBounds: antithetic outer paths are not offered (the martingale is built per outer column): use "
                          "NoVarianceReduction()")
    if int(method.inner) <= 0 or int(method.inner) % 64:
        raise MethodError(f"DualBounds: inner ({method.inner}) must be a multiple of 64 and >= 64")
    fit_seeds = np.asarray(lsm.mc_method.config.seeds, dtype=np.uint64)
    fresh = _seed_set(method.fresh if method.fresh is not None else lsm.mc_method.config.trajectories, int(fit_seeds.max()), "fresh")
    outer = _seed_set(method.outer, int(max(fit_seeds.max(), fresh.max())), "outer")
    _refuse_shared_seeds("DualBounds: the fresh", fresh, fit_seeds)
    _refuse_shared_seeds("DualBounds: the outer", outer, fit_seeds)
    policy = fit_policy(prob, lsm, exercise_every, "spot_variance", path_state)
    low = policy_value(prob, lsm, policy, seeds=fresh, path_state=path_state)
    up = upper_bound(prob, lsm, policy, outer, method.inner, method.inner_seed)
    ins = policy.in_sample
    return BoundsSolution(prob, method, low.price, low.std_error, up.upper, up.upper_se, ins.price, ins.std_error,
                          up.upper - low.price, float(np.hypot(up.upper_se, low.std_error)), policy, up)


@dataclass(frozen=True)
class HestonExactPaths:
    """What simulate_paths(sde_problem(prob, HestonDynamics(), HestonBroadieKaya()), method,
    NoVarianceReduction()) holds per trajectory (montecarlo.jl:209-231, 342-353): the state at the
    steps+1 dates, here as two (steps+1, trajectories) matrices.  `log_spot` is the first state
    component of the reference's solution objects."""
    spot: Any
    variance: Any
    times: Any
    result: Any = field(default=None, compare=False, repr=False)

    @property
    def log_spot(self):
        return np.log(self.spot)


def simulate_heston_exact_paths(prob: PricingProblem, mc: MonteCarlo) -> HestonExactPaths:
    """Per-date Broadie–Kaya transitions (HestonNoise, heston.jl:82-91) through hh_heston_exact_grid."""
    if not (isinstance(mc.dynamics, HestonDynamics) and isinstance(mc.strategy, HestonBroadieKaya)):
        raise MethodError("simulate_heston_exact_paths needs HestonDynamics + HestonBroadieKaya")
    model, c, T = _lsm_structs(prob, mc)
    n, steps = mc.config.trajectories, mc.config.steps
    spot = np.empty((steps + 1, n))
    var = np.empty((steps + 1, n))
    res = _ffi.hh_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_heston_exact_grid(ctx.handle, C.byref(model), C.byref(c), spot.ctypes.data,
                                           var.ctypes.data, 0, C.byref(res)))
    return HestonExactPaths(spot, var, np.linspace(0.0, T, steps + 1), res)


@dataclass(frozen=True)
class EulerPaths:
    """What simulate_paths(sde_problem(prob, dynamics, EulerMaruyama()), method, variance_reduction) holds per
    trajectory (montecarlo.jl:161-207, 342-375), as (steps+1, n) matrices: `spot` in the path state asked for
    (exp(log S), or log S itself), `variance` the Heston variance state (None for lognormal dynamics).  Antithetic:
    n = 2·trajectories, the mirrored path of trajectory i in column trajectories + i."""
    spot: Any
    variance: Any
    times: Any
    result: Any = field(default=None, compare=False, repr=False)


def simulate_euler_paths(prob: PricingProblem, mc: MonteCarlo, path_state: str = "spot") -> EulerPaths:
    """Euler–Maruyama paths (GENERATE) through hh_euler_grid: the draws of solve(prob, mc) on the same seeds, so
    the last spot row is that solve's terminal sample."""
    state = _path_state_code(path_state)
    if not _is_euler(mc):
        raise MethodError("simulate_euler_paths needs LognormalDynamics or HestonDynamics + EulerMaruyama")
    model, c, T = _lsm_structs(prob, mc, euler=True)
    steps = mc.config.steps
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    spot = np.empty((steps + 1, ntot))
    var = np.empty((steps + 1, ntot)) if c.dynamics == _ffi.HH_HESTON else None
    res = _ffi.hh_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_euler_grid(ctx.handle, C.byref(model), C.byref(c), state, spot.ctypes.data,
                                    var.ctypes.data if var is not None else None, 0, C.byref(res)))
    return EulerPaths(spot, var, np.linspace(0.0, T, steps + 1), res)


@dataclass(frozen=True)
class SpotPaths:
    """The spots of a spot-path model's trajectories on every exercise_every-th step, as a (steps/exercise_every + 1, n)
    matrix whose row j lies at times[j]; row 0 is the spot.  Antithetic: n = 2·trajectories, the mirror of trajectory i in
    column trajectories + i."""
    spot: Any
    times: Any
    result: Any = field(default=None, compare=False, repr=False)


def simulate_spot_paths(prob: PricingProblem, mc: MonteCarlo, exercise_every=1) -> SpotPaths:
    """The date rows of solve(prob, mc)'s trajectories through hh_mc_path_grid, on the same seeds: Merton jumps on Euler
    paths, HestonQE, Bates, local volatility, Variance Gamma — the route's own dynamics, inputs and strategy — and the Euler
    paths of the plain models.  The last row is that solve's sample at expiry."""
    m = prob.market_inputs
    route = routes().lsm_route_of(m, mc)
    if route is not None:
        source, model, c, T, n_dates = _source_structs(prob, mc, route, exercise_every)
    elif _is_euler(mc):
        if mc.devices is not None:
            raise MethodError("LSM on Euler paths is not sharded over several GPUs")
        model, c, T = _lsm_structs(prob, mc, euler=True)
        n_dates = _exercise_dates(mc.config.steps, exercise_every)
        source = _ffi.make_path_source(routes().EULER.source)
    else:
        raise MethodError("simulate_spot_paths needs a spot-path model on its own dynamics, inputs and strategy (Merton + "
                          "EulerMaruyama, HestonQE, Bates, local volatility, Variance Gamma) or LognormalDynamics / "
                          "HestonDynamics + EulerMaruyama")
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    spot = np.empty((n_dates + 1, ntot))
    res = _ffi.hh_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_mc_path_grid(ctx.handle, C.byref(source), C.byref(model), C.byref(c), int(exercise_every),
                                      spot.ctypes.data, 0, C.byref(res)))
    return SpotPaths(spot, np.linspace(0.0, T, n_dates + 1), res)


@dataclass(frozen=True)
class StatePaths:
    """The spots and variances of a stochastic-volatility walk on every exercise_every-th step, as two (steps/exercise_every
    + 1, n) matrices whose row j lies at times[j]; row 0 is (spot, V0).  `variance` is the walk's own state: under
    EulerMaruyama the full-truncation scheme's unclipped variance, which can be negative.  Antithetic: n = 2·trajectories,
    the mirror of trajectory i in column trajectories + i."""
    spot: Any
    variance: Any
    times: Any
    result: Any = field(default=None, compare=False, repr=False)


def simulate_state_paths(prob: PricingProblem, mc: MonteCarlo, exercise_every=1) -> StatePaths:
    """The (log S, V) rows of solve(prob, mc)'s trajectories through hh_mc_path_states, on the same seeds: HestonDynamics +
    EulerMaruyama, HestonQE and Bates.  The last spot row is that solve's sample at expiry."""
    source, model, c, T, n_dates = _state_structs(prob, mc, exercise_every)
    ntot = mc.config.trajectories * (2 if c.antithetic else 1)
    rows = np.empty((n_dates + 1, 2, ntot))
    res = _ffi.hh_result()
    ctx = _ffi.get_context(mc.device)
    ctx.check(ctx.lib.hh_mc_path_states(ctx.handle, C.byref(source), C.byref(model), C.byref(c), int(exercise_every),
                                        rows.ctypes.data, 0, C.byref(res)))
    spot, var = _states_of(rows)
    return StatePaths(spot, var, np.linspace(0.0, T, n_dates + 1), res)
