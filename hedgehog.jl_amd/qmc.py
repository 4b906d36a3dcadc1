"""Randomised quasi-Monte Carlo: `solve(problem, QuasiMonteCarlo(dynamics, strategy, SobolConfig(...)))`.

No reference method.  Each randomisation is one digital shift of the same Sobol' points: hh_sobol_fill writes its
increments into one device buffer in the tile-major REPLAY layout, and the REPLAY form of hh_mc_solve — the kernels every
Monte Carlo solve runs — prices on it.  The price is the mean of the randomisations' estimates, its standard error their
sample standard deviation over √R (include/hedgehog_mc.h, "Quasi-Monte Carlo").  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import _ffi
from .domain import PATH_PAYOFFS, American, BlackScholesInputs, European, HestonInputs, PricingProblem, Spot, VanillaOption
from .dual import value_of
from .montecarlo import (AbstractPricingMethod, BlackScholesExact, EulerMaruyama, HestonDynamics, LognormalDynamics,
                         MethodError, NoVarianceReduction, _model_and_config, _price_from)


class BrownianBridge: pass   # HH_SOBOL_BRIDGE: the first coordinates carry the terminal values
class Incremental: pass      # HH_SOBOL_INCREMENTAL: coordinate ncomp·step + comp is that increment

for _c in (BrownianBridge, Incremental):
    _c.__eq__ = lambda a, b: type(a) is type(b)
    _c.__hash__ = lambda a: hash(type(a).__name__)
    _c.__repr__ = lambda a: type(a).__name__ + "()"

SUPPORTED = ("QuasiMonteCarlo prices European vanilla options on Spot with (LognormalDynamics, BlackScholesExact), "
             "(LognormalDynamics, EulerMaruyama) on BlackScholesInputs or (HestonDynamics, EulerMaruyama) on HestonInputs, "
             "on one device")


class SobolConfig:
    """`SobolConfig(points, steps=1, randomizations=16, seed=None, construction=BrownianBridge())`: R digital shifts,
    drawn from `seed` (a random one when None — fix it to price bumped problems on the same points), of the first
    `points` Sobol' points.  A power of two keeps the point set a net."""

    def __init__(self, points, steps=1, randomizations=16, seed=None, construction=None):
        self.points, self.steps, self.randomizations = int(points), int(steps), int(randomizations)
        if not 1 <= self.points <= 2 ** 32 - 256:
            raise ValueError(f"SobolConfig: 1 .. 2^32 - 256 points, not {points}")
        if self.steps < 1 or self.randomizations < 1:
            raise ValueError("SobolConfig: steps and randomizations must be at least 1")
        self.seed = int(np.random.default_rng().integers(0, 2 ** 64, dtype=np.uint64)) if seed is None else int(seed) % 2 ** 64
        self.construction = BrownianBridge() if construction is None else construction
        if not isinstance(self.construction, (BrownianBridge, Incremental)):
            raise ValueError("SobolConfig: construction is BrownianBridge() or Incremental()")

    # what montecarlo._model_and_config reads of a SimulationConfig
    @property
    def trajectories(self):
        return self.points

    variance_reduction = NoVarianceReduction()


@dataclass(frozen=True)
class QuasiMonteCarlo(AbstractPricingMethod):
    """The method of a randomised QMC solve; em_split / compat_sqrt_alpha / device as MonteCarlo's."""
    dynamics: Any
    strategy: Any
    config: SobolConfig
    em_split: bool = True
    compat_sqrt_alpha: bool = False
    device: int = 0
    devices: Any = None  # refused: one device


@dataclass(frozen=True)
class QuasiMonteCarloSolution:
    """price: the mean of `estimates` (one per randomisation; Duals where the problem carries them); std_error: their
    sample standard deviation over √R, NaN for R = 1."""
    problem: Any
    method: Any
    price: Any
    std_error: float = float("nan")
    estimates: Any = field(default=())


def summarize(estimates):
    """(mean, standard error) of the randomisations' estimates"""
    R = len(estimates)
    total = estimates[0]
    for e in estimates[1:]:
        total = total + e
    vals = np.array([value_of(e) for e in estimates], dtype=np.float64)
    se = float(vals.std(ddof=1)) / math.sqrt(R) if R > 1 else float("nan")
    return total / R, se


def check_supported(prob: PricingProblem, method: QuasiMonteCarlo):
    """a MethodError that names what is supported, for everything else"""
    payoff, m, dyn, strat = prob.payoff, prob.market_inputs, method.dynamics, method.strategy
    if method.devices is not None:
        raise MethodError(f"QuasiMonteCarlo does not shard over devices=: {SUPPORTED}")
    if isinstance(payoff, PATH_PAYOFFS):
        raise MethodError(f"{type(payoff).__name__}: the path-statistics family draws its own noise (no REPLAY): {SUPPORTED}")
    if isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, American):
        raise MethodError(f"American exercise is priced by LSM, which draws its own paths: {SUPPORTED}")
    if not (isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European) and
            isinstance(payoff.underlying, Spot)):
        raise MethodError(f"{type(payoff).__name__}: {SUPPORTED}")
    ok = (isinstance(dyn, LognormalDynamics) and type(strat) in (BlackScholesExact, EulerMaruyama) and
          isinstance(m, BlackScholesInputs)) or \
         (isinstance(dyn, HestonDynamics) and type(strat) is EulerMaruyama and isinstance(m, HestonInputs))
    if not ok:
        raise MethodError(f"no quasi-Monte Carlo route for {type(dyn).__name__} + {type(strat).__name__} on "
                          f"{type(m).__name__}: {SUPPORTED}")
    if not isinstance(method.config, SobolConfig):
        raise MethodError(f"QuasiMonteCarlo takes a SobolConfig, not a {type(method.config).__name__}: {SUPPORTED}")


def solve_qmc(prob: PricingProblem, method: QuasiMonteCarlo) -> QuasiMonteCarloSolution:
    check_supported(prob, method)
    cfg = method.config
    model, c, keep, P, discount = _model_and_config(prob, method)
    euler = c.strategy == _ffi.HH_EULER_MARUYAMA
    # the exact law reads one standard normal per point: a lognormal fill of one step over T = 1
    dyn, steps, T = (c.dynamics, cfg.steps, model.T) if euler else (_ffi.HH_LOGNORMAL, 1, 1.0)
    construction = _ffi.HH_SOBOL_BRIDGE if isinstance(cfg.construction, BrownianBridge) else _ffi.HH_SOBOL_INCREMENTAL
    ctx = _ffi.get_context(method.device)
    n_elems = ctx.lib.hh_replay_elems(cfg.points, steps, dyn)
    buf = _ffi.DeviceBuffer(ctx, 8 * n_elems, pooled=True)  # one buffer, refilled per randomisation
    c.noise_mode, c.replay_layout = _ffi.HH_NOISE_REPLAY, _ffi.HH_REPLAY_TILE_MAJOR
    c.replay, c.replay_on_device, c.replay_len = buf.ptr, 1, n_elems
    estimates = []
    try:
        for r in range(cfg.randomizations):
            ctx.check(ctx.lib.hh_sobol_fill(ctx.handle, dyn, model.rho, T, steps, cfg.points, 0, cfg.seed, r, 1, construction,
                                            buf.ptr))
            res = _ffi.hh_result()
            ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(model), C.byref(c), C.byref(res), None))
            estimates.append(_price_from(res, discount, P))
    finally:
        buf.recycle()
    del keep
    price, se = summarize(estimates)
    return QuasiMonteCarloSolution(prob, method, price, se, tuple(estimates))
