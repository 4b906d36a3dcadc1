"""The Monte Carlo routes of the host, each stated once: what claims a (payoffs, market inputs, method) triple, what the
route admits, what its C structs are formed on, its entry point, what it refuses and in which words, and what a basket
does with the payoffs no path group took.  montecarlo.solve_montecarlo, solve_montecarlo_many, solve_path_payoffs and
basket.solve_basket look a triple up here (route_of) and act on the record; hh.solve turns the other methods away by it.

A new model is one Route in ROUTES, before the routes it must win against.  Where its structs are not those of a European
solve on some plain market (several assets: multiasset.py), it forms them itself and hands them to montecarlo.run_paths.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Any, Callable

from . import _ffi
from .analytic import CarrMadan, VarianceGammaAnalytic
from .domain import (PATH_PAYOFFS, American, BatesInputs, ContinuousMonitoring, European, HestonInputs, MertonInputs,
                     PricingProblem, Spot, VanillaOption, VarianceGammaInputs)
from .dual import Dual
from .localvol import ROUTES as LOCALVOL_ROUTES, LocalVolDynamics, LocalVolInputs, is_localvol
from .montecarlo import (BATES_ROUTES, BatesDynamics, BlackScholesExact, EulerMaruyama, HestonDynamics, HestonQE,
                         LognormalDynamics, MertonDynamics, MertonExact, MethodError, MonteCarlo, VG_ROUTES,
                         VarianceGammaDynamics, VarianceGammaExact, _model_and_config, is_bates, is_merton, is_qe, is_vg)
from .multiasset import ROUTES as ASSET_ROUTES, MultiAssetDynamics, MultiAssetInputs, is_multiasset, solve_index_options

# ---- what a path route may refuse before the expiry and the monitoring of its payoffs are looked at (Route.early) ----

def admitted(route, payoffs, m, method):
    dyn, strat = method.dynamics, method.strategy
    D, M, S = route.admits
    if not (isinstance(dyn, D) and isinstance(m, M) and isinstance(strat, S)):
        raise MethodError(route.not_admitted.format(dyn=type(dyn).__name__, strat=type(strat).__name__, m=type(m).__name__))


def european_discrete(route, payoffs, m, method):
    for p in payoffs:
        if route.no_american and isinstance(getattr(p, "exercise_style", None), American):
            raise MethodError(route.no_american)
        if route.no_continuous and isinstance(getattr(p, "monitoring", None), ContinuousMonitoring):
            raise MethodError(route.no_continuous)


def euler_paths(route, payoffs, m, method):
    if not isinstance(method.strategy, EulerMaruyama):
        raise MethodError(f"path-dependent payoffs need EulerMaruyama paths, not {type(method.strategy).__name__}")


def one_device(route, payoffs, m, method):
    if method.devices is not None:
        raise MethodError(route.one_device)


@dataclass(frozen=True)
class Route:
    name: str
    claims: Callable                 # (payoffs, market_inputs, method) -> bool; the first route that claims a triple has it
    # ---- what it admits, and the structs: hh_model, extras …, hh_config in the C argument order ----
    admits: Any = None               # (dynamics, inputs, strategies) types; None: _model_and_config decides, in its own words
    not_admitted: str = None         # the MethodError of a claimed triple that is not admitted: {dyn}, {strat}, {m}
    base: Callable = None            # (market_inputs, method) -> the plain (market, method) hh_model / hh_config are formed on
    strategy: Any = None             # enum hh_strategy written over the plain method's
    dual_fields: tuple = ()          # fields of the inputs that the plain market does not carry: no Dual in them
    extras: Callable = None          # (market_inputs, method) -> the structs the route brings
    # ---- the entry point ----
    entry: str = None                # hh_mc_solve_path*, or the terminal law's; None: hh_mc_solve and its kin
    takes_extremes: bool = False     # the call carries enum hh_path_extremes after include_start
    entry_ex: str = None             # the entry point (with extremes) of a lookback or a continuously monitored payoff
    tail: tuple = ()                 # NULLs after the statistics (var_T)
    law: bool = False                # `entry` samples the law at expiry: one European vanilla, no paths
    source: int = None               # enum hh_path_source_kind: the route's paths as date rows (hh_mc_path_grid, LSM on them)
    solve_all: Callable = None       # (payoffs, market_inputs, method, ensemble): a grouping of its own, for one payoff or many
    own_lsm: bool = False            # an LSM on the route's own triple has an induction of its own (no date rows of one spot)
    state_rows: bool = False         # the walk holds a variance: (log S, V) rows (hh_mc_path_states) and an LSM on (S, V)
    nested_walk: bool = False        # the walk restarts from stored (log S, V) states: the dual upper bound (hh_lsm_upper_bound)
    # ---- what it refuses, and in which words ----
    early: tuple = ()                # of the four checks above, in the route's order; `admitted` elsewhere: with the structs
    no_replay: str = None
    one_device: str = None
    no_duals: str = None
    no_american: str = None
    no_continuous: str = None        # a payoff under ContinuousMonitoring(), early
    no_bridge: str = None            # the bridge mode, once the structs stand
    no_paths: str = None             # a path-dependent payoff on the law at expiry
    methods: tuple = (MonteCarlo,)   # the methods that price the model; hh.solve turns every other one away with
    other_methods: str = None        # "{} does not price …: use …" (None: nothing is turned away)
    # ---- baskets and batches ----
    rest: str = "terminal"           # the payoffs no path group took: "terminal" (hh_mc_solve_basket), "paths" (one simulation
    checks_first: bool = False       # per expiry), "singles"; checks_first: the first payoff's refusals before any grouping
    multi: bool = False              # an hh_mc_solve_multi form

    def takes_lsm(self, m, mc):
        """Is `mc` — the MonteCarlo method inside an LSM — this route's own triple?  Then LSM regresses on its date rows."""
        if (self.source is None and not self.own_lsm) or self.admits is None or not self.claims((), m, mc):
            return False
        D, M, S = self.admits
        return isinstance(mc.dynamics, D) and isinstance(m, M) and isinstance(mc.strategy, S)

    def refuse_method(self, payoffs, m, method):
        mc = getattr(method, "mc_method", None)  # an LSM: on the route's own triple it is one of the route's methods
        if mc is not None and self.takes_lsm(m, mc):
            return
        if self.other_methods and not isinstance(method, self.methods) and self.claims(payoffs, m, method):
            raise MethodError(self.other_methods.format(type(method).__name__))

    def form_structs(self, payoff, m, method):
        """(hh_model, hh_config, extras) of a European solve of `payoff` (a path solve: its expiry alone is read) on the
        route's plain market; whatever the route does not admit, a second device and a Dual anywhere are MethodErrors."""
        if self.admits and admitted not in self.early:
            admitted(self, None, m, method)
        if method.devices is not None:
            raise MethodError(self.one_device)
        for f in self.dual_fields:
            if isinstance(getattr(m, f), Dual):
                raise MethodError(self.no_duals)
        market, plain = self.base(m, method) if self.base else (m, method)
        model, c, _, P, _ = _model_and_config(PricingProblem(payoff, market), plain)
        if P:  # the policy of every full-path entry point: never drop partials silently
            raise MethodError(self.no_duals)
        if self.strategy is not None:
            c.strategy = self.strategy
        return model, c, self.extras(m, method) if self.extras else ()


def _jump(m, method):
    return (_ffi.make_jump(float(m.jump_intensity), float(m.jump_mean), float(m.jump_std)),)


def _vg(m, method):
    return (_ffi.make_vg(float(m.theta), float(m.nu)),)


def _one_european_vanilla(payoffs):
    p = payoffs[0] if len(payoffs) == 1 else None
    return isinstance(p, VanillaOption) and isinstance(p.exercise_style, European) and isinstance(p.underlying, Spot)


def _qe(m, method):
    return (_ffi.make_qe(float(method.strategy.psi_c), bool(method.strategy.martingale)),)


def _on_lognormal(**kw):
    return lambda m, method: (m.black_scholes(), dataclasses.replace(method, dynamics=LognormalDynamics(), **kw))


JUMPS = ("jump_intensity", "jump_mean", "jump_std")

MULTIASSET = Route(
    "multi-asset", is_multiasset,
    admits=(MultiAssetDynamics, MultiAssetInputs, EulerMaruyama),
    not_admitted="no multi-asset solve for {dyn} + {strat} on {m}: use " + ASSET_ROUTES,
    entry="hh_mc_solve_path_assets", solve_all=solve_index_options, own_lsm=True,
    no_replay="multi-asset solves draw their own noise: no replay",
    one_device="multi-asset solves run on one device (MonteCarlo.devices is not supported)",
    no_duals="multi-asset solves carry no dual partials (ForwardAD): use FiniteDifference with AssetSpotLens, AssetVolLens or "
             "CorrelationLens — its solves share their seeds",
    no_american="American exercise is not offered on an index of several assets: European payoffs on " + ASSET_ROUTES,
    no_continuous="ContinuousMonitoring() is not offered on an index of several assets (no bridge form): monitor on the dates of "
                  "a Monitoring",
    other_methods="{} does not price multi-asset problems: use " + ASSET_ROUTES)

LOCALVOL = Route(
    "local volatility", lambda payoffs, m, method: is_localvol(m, method),
    admits=(LocalVolDynamics, LocalVolInputs, EulerMaruyama),
    not_admitted="no local-volatility solve for {dyn} + {strat} on {m}: use " + LOCALVOL_ROUTES,
    base=_on_lognormal(), dual_fields=("spot",), extras=lambda m, method: (m.surface.c_struct(),),
    entry="hh_mc_solve_path_lv", takes_extremes=True, source=_ffi.HH_SOURCE_LOCALVOL, early=(admitted, european_discrete, one_device),
    no_replay="local-volatility solves draw their own noise: no replay",
    one_device="local-volatility solves run on one device (MonteCarlo.devices is not supported)",
    no_duals="local-volatility solves carry no dual partials (ForwardAD): use FiniteDifference — its solves share their seeds, "
             "the spot or the curve moves and the surface stays",
    no_american="American exercise is not offered on local-volatility paths (no LSM on them): European payoffs on " + LOCALVOL_ROUTES,
    other_methods="{} does not price local volatility: use " + LOCALVOL_ROUTES, rest="paths", checks_first=True)

BATES = Route(
    "Bates", lambda payoffs, m, method: is_bates(m, method),
    admits=(BatesDynamics, BatesInputs, HestonQE), not_admitted="no Bates solve for {dyn} + {strat} on {m}: use " + BATES_ROUTES,
    base=lambda m, method: (m.heston(), dataclasses.replace(method, dynamics=HestonDynamics(), strategy=EulerMaruyama())),
    strategy=_ffi.HH_QE, dual_fields=JUMPS, extras=lambda m, method: _qe(m, method) + _jump(m, method),
    entry="hh_mc_solve_path_bates", tail=(None,), source=_ffi.HH_SOURCE_BATES, state_rows=True, early=(admitted, european_discrete, one_device),
    no_replay="Bates solves draw their own noise: no replay",
    one_device="path-dependent payoffs run on one device (MonteCarlo.devices is not supported)",
    no_duals="Bates solves carry no dual partials (ForwardAD): use FiniteDifference — its solves share their seeds",
    no_american="American exercise is not offered on Bates paths (no LSM on them): European payoffs on " + BATES_ROUTES,
    no_continuous="ContinuousMonitoring() is not offered on Bates paths (a bridge between two states is wrong once a jump lies "
                  "between them): monitor on the dates of a Monitoring",
    methods=(MonteCarlo, CarrMadan), other_methods="{} does not price the Bates model: use " + BATES_ROUTES, rest="paths")

QE = Route(
    "HestonQE", lambda payoffs, m, method: is_qe(method),
    admits=(HestonDynamics, HestonInputs, HestonQE),
    not_admitted="HestonQE simulates HestonDynamics() on HestonInputs, not {dyn} on {m}: use EulerMaruyama or the model's exact "
                 "strategy there",
    base=lambda m, method: (m, dataclasses.replace(method, strategy=EulerMaruyama())), strategy=_ffi.HH_QE, extras=_qe,
    entry="hh_mc_solve_path_qe", tail=(None,), source=_ffi.HH_SOURCE_QE, state_rows=True, early=(european_discrete, one_device),
    no_replay="HestonQE solves draw their own noise: no replay (EulerMaruyama takes one)",
    one_device="path-dependent payoffs run on one device (MonteCarlo.devices is not supported)",
    no_duals="HestonQE solves carry no dual partials (ForwardAD): use FiniteDifference — its solves share their seeds",
    no_american="American exercise is not offered on HestonQE paths: use LSM(HestonDynamics(), EulerMaruyama() | "
                "HestonBroadieKaya(), …)",
    no_continuous="ContinuousMonitoring() is not offered on HestonQE paths (the step's interpolation is no frozen-coefficient "
                  "bridge): monitor on the dates of a Monitoring, or use EulerMaruyama()",
    rest="paths")

MERTON = Route(  # Merton jumps on Euler paths
    "Merton paths", lambda payoffs, m, method: is_merton(m, method) and isinstance(getattr(method, "strategy", None), EulerMaruyama),
    admits=(MertonDynamics, MertonInputs, (EulerMaruyama, MertonExact)),
    not_admitted="no sde_problem / marginal_law for {dyn} + {strat} on {m}",
    base=_on_lognormal(compat_sqrt_alpha=False), dual_fields=JUMPS, extras=_jump,
    entry="hh_mc_solve_path_jump", source=_ffi.HH_SOURCE_JUMP, early=(one_device,),
    no_replay="Merton solves draw their own noise: no replay",
    one_device="path-dependent payoffs run on one device (MonteCarlo.devices is not supported)",
    no_duals="Merton solves carry no dual partials: use FiniteDifference",
    no_bridge="ContinuousMonitoring is not offered under Merton jumps: monitor on the dates of a Monitoring",
    rest="paths")

MERTON_LAW = dataclasses.replace(  # MertonExact: the law at expiry (and whatever else a Merton pair names: not admitted)
    MERTON, name="Merton law", claims=lambda payoffs, m, method: is_merton(m, method),
    base=_on_lognormal(compat_sqrt_alpha=False, strategy=BlackScholesExact()), entry="hh_mc_solve_jump", law=True, source=None,
    early=(euler_paths,),  # asked for paths (a basket's path groups): refused
    one_device="Merton solves run on one device (MonteCarlo.devices is not supported)", no_bridge=None,
    no_paths="MertonExact samples the law at expiry: path-dependent payoffs need EulerMaruyama paths", rest="singles")

VG = Route(  # Variance Gamma: every payoff on the path statistics, exact in law on any dates
    "Variance Gamma paths", lambda payoffs, m, method: is_vg(m, method),
    admits=(VarianceGammaDynamics, VarianceGammaInputs, VarianceGammaExact),
    not_admitted="no Variance Gamma solve for {dyn} + {strat} on {m}: use " + VG_ROUTES,
    base=_on_lognormal(compat_sqrt_alpha=False, strategy=BlackScholesExact()), dual_fields=("theta", "nu"), extras=_vg,
    entry="hh_mc_solve_path_vg", source=_ffi.HH_SOURCE_VG, early=(admitted, european_discrete, one_device),
    no_replay="Variance Gamma solves draw their own noise (gamma variates by rejection): no replay; use " + VG_ROUTES,
    one_device="Variance Gamma solves run on one device (MonteCarlo.devices is not supported): use " + VG_ROUTES,
    no_duals="Variance Gamma solves carry no dual partials (ForwardAD): use FiniteDifference with SpotLens, VolLens, "
             "optic(\"market_inputs.theta\") or optic(\"market_inputs.nu\") — its solves share their seeds",
    no_american="American exercise is not offered on Variance Gamma paths (no LSM on them): European payoffs on " + VG_ROUTES,
    no_continuous="ContinuousMonitoring() is not offered on Variance Gamma paths (between two dates the path is no diffusion "
                  "bridge): monitor on the dates of a Monitoring",
    methods=(MonteCarlo, CarrMadan, VarianceGammaAnalytic), other_methods="{} does not price the Variance Gamma model: use " + VG_ROUTES,
    rest="paths")

VG_LAW = dataclasses.replace(  # one European vanilla on the spot: the law at expiry, one gamma variate per trajectory
    VG, name="Variance Gamma law", claims=lambda payoffs, m, method: is_vg(m, method) and _one_european_vanilla(payoffs),
    entry="hh_mc_solve_vg", law=True, source=None, early=(), rest="singles")

EULER = Route(  # a path-dependent payoff on the Euler paths of the plain models; vanillas of its basket: the plain route's
    "Euler paths", lambda payoffs, m, method: any(isinstance(p, PATH_PAYOFFS) for p in payoffs),
    entry="hh_mc_solve_path", entry_ex="hh_mc_solve_path_ex", source=_ffi.HH_SOURCE_EULER, nested_walk=True,
    early=(euler_paths, one_device),
    no_replay="path-dependent payoffs draw their own noise: no replay",
    one_device="path-dependent payoffs run on one device (MonteCarlo.devices is not supported)",
    no_duals="path-dependent payoffs carry no dual partials: use FiniteDifference")

PLAIN = Route("plain European", lambda payoffs, m, method: True, multi=True)  # hh_mc_solve, _basket, _multi; replay, devices, duals

ROUTES = (MULTIASSET, LOCALVOL, BATES, QE, VG_LAW, VG, MERTON, MERTON_LAW, EULER, PLAIN)
SPOT_PATHS = (LOCALVOL, BATES, QE, VG, MERTON)  # what solve_path_payoffs looks a pair up in; whatever none claims: EULER
OTHER_METHODS = (MULTIASSET, BATES, LOCALVOL, VG)  # in the order hh.solve asks them


def route_of(payoffs, market_inputs, method, routes=ROUTES) -> Route:
    for route in routes:
        if route.claims(payoffs, market_inputs, method):
            return route


def path_route_of(payoffs, market_inputs, method) -> Route:
    return route_of(payoffs, market_inputs, method, SPOT_PATHS) or EULER


def lsm_route_of(market_inputs, mc) -> Route:
    """The route whose date rows an LSM on `mc` regresses on: the one that takes the triple as its own, or None (the Euler and
    exact sources of lsm.py, and every refusal there)."""
    for route in SPOT_PATHS:
        if route.takes_lsm(market_inputs, mc):
            return route


STATE_ROWS = "HestonDynamics() + EulerMaruyama() (under path_state=\"spot\"), HestonQE and Bates"  # the walks with a variance


NESTED_WALKS = "HestonDynamics() + EulerMaruyama()"  # the walks hh_lsm_upper_bound restarts from stored states


def bounds_route_of(market_inputs, mc) -> Route:
    """The route whose walk serves DualBounds on `mc`: the lower bound needs state rows, the upper bound a nested walk.  A route
    that cannot serve raises MethodError naming what is missing."""
    if own_lsm_route_of(market_inputs, mc) is not None:
        raise MethodError("DualBounds: the several-asset walk has no variance rows and no nested walk; the bounds need " + NESTED_WALKS)
    route = lsm_route_of(market_inputs, mc)
    if route is None:
        if isinstance(mc.strategy, EulerMaruyama) and isinstance(mc.dynamics, HestonDynamics):
            return EULER
        raise MethodError(f"DualBounds: {type(mc.dynamics).__name__} + {type(mc.strategy).__name__} has no variance rows and no "
                          "nested walk; the bounds need " + NESTED_WALKS)
    if not route.state_rows:
        raise MethodError(f"DualBounds: the walk of {route.name} has no variance rows (and no nested walk); the bounds need "
                          + NESTED_WALKS)
    if not route.nested_walk:
        raise MethodError(f"DualBounds: {route.name} has state rows (fit_policy and policy_value serve it) but no nested walk: "
                          "the upper bound needs " + NESTED_WALKS)
    return route


def own_lsm_route_of(market_inputs, mc) -> Route:
    """The route that prices an LSM on `mc` by an induction of its own (several assets: several state rows per date), or None"""
    return MULTIASSET if MULTIASSET.takes_lsm(market_inputs, mc) else None


def path_source(route, extras):
    """hh_path_source of a route over the structs it brought (Route.extras), each in the field of its type"""
    fields = {_ffi.hh_jump: "jump", _ffi.hh_qe: "qe", _ffi.hh_localvol: "localvol", _ffi.hh_vg: "vg"}
    return _ffi.make_path_source(route.source, **{fields[type(x)]: x for x in extras})


def refuse_other_methods(payoffs, market_inputs, method):
    """"<method> does not price <model>: use <its routes>" for every model that has only routes of its own"""
    for route in OTHER_METHODS:
        route.refuse_method(payoffs, market_inputs, method)
