"""Host mirror of /root/reference/src/calibration/basket.jl: `BasketPricingProblem`,
`BasketPricingSolution` and `solve(::BasketPricingProblem, ::MonteCarlo)`.

The reference prices a basket as independent solves (basket.jl:35-38).  With the fixed seeds of
`SimulationConfig`, payoffs that share an expiry see the same trajectories, so here every expiry
group is ONE simulation whose terminal samples are reduced against all of the group's strikes
(`hh_mc_solve_basket`).  Results equal the per-payoff solves (tests/test_gpu_basket.py).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _ffi
from .domain import PATH_PAYOFFS, European, MonteCarloSolution, PricingProblem, Spot, VanillaOption
from .dual import Dual
from .montecarlo import (_model_and_config, _path_structs, _price_from, path_extremes, path_monitoring, routes, solve_montecarlo,
                         solve_path_payoffs)


@dataclass(frozen=True)
class BasketPricingProblem:
    """basket.jl:10-13."""
    payoffs: Any
    market_inputs: Any


@dataclass(frozen=True)
class BasketPricingSolution:
    """basket.jl:24-27."""
    problem: BasketPricingProblem
    solutions: Any


def path_groups(payoffs, steps):
    """The path solves of a basket: [((expiry, monitoring), [indices])], in order of first appearance.  Path-dependent
    payoffs are grouped by (expiry, monitoring).  A payoff that reads the state at expiry alone — a digital, a European
    vanilla on the spot — rides along with the first group of its expiry; digitals of an expiry without one form a
    group of their own (monitored at expiry), vanillas of such an expiry are left to the terminal-sample basket.
    A group also shares its extremes mode.  A continuously monitored barrier or lookback has no dates of its own: it
    joins the first group of its expiry in which nothing reads the extremes of the dates (no discrete barrier or
    lookback: a group of Asians, say), and otherwise the expiry's group without dates, with the digitals."""
    groups: dict = {}
    for i, p in enumerate(payoffs):
        if isinstance(p, PATH_PAYOFFS) and path_monitoring(p, steps) is not None:
            groups.setdefault((p.expiry, path_monitoring(p, steps)), []).append(i)
    for i, p in enumerate(payoffs):
        if path_extremes(p) == _ffi.HH_EXTREMES_BRIDGE:
            key = next((k for k, idx in groups.items() if k[0] == p.expiry and k[1] is not None and
                        all(path_extremes(payoffs[j]) is None for j in idx)), (p.expiry, None))
            groups.setdefault(key, []).append(i)
    for i, p in enumerate(payoffs):
        vanilla = isinstance(p, VanillaOption) and isinstance(p.exercise_style, European) and \
            isinstance(p.underlying, Spot) and not isinstance(p.strike, Dual)
        if not (vanilla or (isinstance(p, PATH_PAYOFFS) and path_monitoring(p, steps) is None and path_extremes(p) is None)):
            continue
        key = next((k for k in groups if k[0] == p.expiry and k[1] is not None), None)
        if key is None and not vanilla:
            key = (p.expiry, None)
        if key is not None:
            groups.setdefault(key, []).append(i)
    return [(k, sorted(idx)) for k, idx in groups.items()]


def solve_basket(prob: BasketPricingProblem, method, ensemble: bool = False):
    """basket.jl:35-38 for a MonteCarlo method (one simulation per expiry group), CarrMadan (every
    Fourier integral in one launch), CoxRossRubinsteinMethod (every tree in one launch) or CrankNicolsonMethod
    (every grid in one launch)."""
    from .analytic import AnalyticSolution, CarrMadan, solve_carr_madan_basket
    from .trees import CoxRossRubinsteinMethod, CRRSolution, solve_crr_basket
    from .pde import CrankNicolsonMethod, solve_pde_basket
    route = routes().route_of(prob.payoffs, prob.market_inputs, method)
    if route.solve_all:  # IndexOptions: one statistics pass per distinct index
        return BasketPricingSolution(prob, route.solve_all(prob.payoffs, prob.market_inputs, method, ensemble))
    routes().LOCALVOL.refuse_method(prob.payoffs, prob.market_inputs, method)  # its inputs are no other method's
    if isinstance(method, CoxRossRubinsteinMethod):
        prices = solve_crr_basket(prob.payoffs, prob.market_inputs, method)
        return BasketPricingSolution(prob, [CRRSolution(PricingProblem(p, prob.market_inputs), method, float(x))
                                            for p, x in zip(prob.payoffs, prices)])
    if isinstance(method, CrankNicolsonMethod):
        return BasketPricingSolution(prob, solve_pde_basket(prob.payoffs, prob.market_inputs, method))
    if isinstance(method, CarrMadan):
        prices = solve_carr_madan_basket(prob.payoffs, prob.market_inputs, method)
        return BasketPricingSolution(prob, [AnalyticSolution(PricingProblem(p, prob.market_inputs), method,
                                                             x if isinstance(x, Dual) else float(x))
                                            for p, x in zip(prob.payoffs, prices)])
    payoffs = list(prob.payoffs)
    sols: list = [None] * len(payoffs)
    groups: dict = {}
    if route.checks_first:  # the route's refusals, before anything is grouped
        _path_structs(payoffs[:1], prob.market_inputs, method, route)
    if route.entry:  # a path-dependent payoff, or a model on paths alone: one path solve per (expiry, monitoring)
        for _, idx in path_groups(payoffs, method.config.steps):
            for i, sol in zip(idx, solve_path_payoffs([payoffs[i] for i in idx], prob.market_inputs, method, ensemble, route)):
                sols[i] = sol
    left = [i for i in range(len(payoffs)) if sols[i] is None]
    if route.rest == "singles":  # the law at expiry: the same seed gives the same trajectories
        for i in left:
            sols[i] = solve_montecarlo(PricingProblem(payoffs[i], prob.market_inputs), method, ensemble)
        return BasketPricingSolution(prob, sols)
    if route.rest == "paths":  # no terminal-sample basket: one path simulation per expiry, the vanilla kind
        for i in left:
            groups.setdefault(getattr(payoffs[i], "expiry", None), []).append(i)
        for idx in groups.values():
            for i, sol in zip(idx, solve_path_payoffs([payoffs[i] for i in idx], prob.market_inputs, method, ensemble, route)):
                sols[i] = sol
        return BasketPricingSolution(prob, sols)
    for i in left:
        if isinstance(getattr(payoffs[i], "strike", None), Dual):  # strike partials: plain per-payoff solve
            sols[i] = solve_montecarlo(PricingProblem(payoffs[i], prob.market_inputs), method, ensemble)
        else:
            groups.setdefault(getattr(payoffs[i], "expiry", None), []).append(i)
    cfg = method.config
    mg = _ffi.get_multi_gpu(tuple(method.devices)) if method.devices is not None else None
    ctx = None if mg is not None else _ffi.get_context(method.device)
    for idx in groups.values():
        first = PricingProblem(payoffs[idx[0]], prob.market_inputs)
        model, c, keep, P, discount = _model_and_config(first, method)  # raises MethodError as solve
        for i in idx[1:]:
            _model_and_config(PricingProblem(payoffs[i], prob.market_inputs), method)
        K = len(idx)
        strikes = (C.c_double * K)(*[float(payoffs[i].strike) for i in idx])
        cps = (C.c_double * K)(*[payoffs[i].call_put() for i in idx])
        anti = bool(c.antithetic)
        if mg is not None:  # ONE call, the group's simulation sharded over method.devices (hh_mgpu_solve_basket)
            if ensemble:
                raise ValueError("ensemble=True is not returned by the multi-GPU basket")
            c.seeds, c.seeds_len = cfg.seeds.ctypes.data, cfg.seeds.size
            res = (_ffi.hh_result * K)()
            mg.check(mg.lib.hh_mgpu_solve_basket(mg.handle, C.byref(model), C.byref(c), strikes, cps, K, res))
            for k, i in enumerate(idx):
                sols[i] = MonteCarloSolution(PricingProblem(payoffs[i], prob.market_inputs), method,
                                             _price_from(res[k], discount, P), None,
                                             std_error=res[k].std_error, result=res[k])
            del keep
            continue
        # the context's seed cache: uploaded once per config, not once per objective evaluation
        c.seeds, c.seeds_on_device = cfg.device_seeds(ctx), 1
        c.seeds_len = cfg.seeds.size
        term = np.empty(c.n_paths * (2 if anti else 1)) if ensemble else None
        res = (_ffi.hh_result * K)()
        ctx.check(ctx.lib.hh_mc_solve_basket(ctx.handle, C.byref(model), C.byref(c), strikes, cps, K,
                                             res, term.ctypes.data if ensemble else None))
        ens = None
        if ensemble:
            ens = (term[:c.n_paths], term[c.n_paths:]) if anti else term
        for k, i in enumerate(idx):
            sols[i] = MonteCarloSolution(PricingProblem(payoffs[i], prob.market_inputs), method,
                                         _price_from(res[k], discount, P), ens,
                                         std_error=res[k].std_error, result=res[k])
        del keep
    return BasketPricingSolution(prob, sols)
