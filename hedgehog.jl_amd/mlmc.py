"""Multilevel Monte Carlo (Giles 2008): `solve(problem, MultilevelMonteCarlo(dynamics, EulerMaruyama(), MLMCConfig(...)))`.

No reference method.  The price is the telescoping sum E[P_0] + Σ_{l=1..L} E[P_l − P_{l−1}] over Euler–Maruyama grids of
steps·2^l steps: level 0 is a plain path solve (hh_mc_solve_path / hh_mc_solve_path_ex), every correction one
hh_mc_solve_path_coupled — a fine and a coarse trajectory on the same draws in one kernel (include/hedgehog_mc.h,
"Multilevel Monte Carlo").  The host chooses the levels and the trajectory counts and adds the levels'
sums.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import _ffi
from .domain import (PATH_PAYOFFS, American, BlackScholesInputs, ContinuousMonitoring, European, HestonInputs, LookbackOption,
                     PricingProblem, Spot, VanillaOption)
from .montecarlo import (AbstractPricingMethod, EulerMaruyama, HestonDynamics, LognormalDynamics, MethodError, MonteCarlo,
                         SimulationConfig, _path_structs, pack_path_payoff, path_monitoring, routes)

SUPPORTED = ("MultilevelMonteCarlo prices one European vanilla option on Spot, AsianOption, BarrierOption, DigitalOption or "
             "LookbackOption under a Monitoring, with (LognormalDynamics, EulerMaruyama) on BlackScholesInputs or "
             "(HestonDynamics, EulerMaruyama) on HestonInputs, on one device")

BATCH = 2 ** 22            # trajectories of one library call: a level's count is run in batches of at most this many
MAX_STEPS = 4 * 65535      # the library's bound on the steps of an Euler solve
CORRECTION_COST = 1.5      # a correction steps a fine and a coarse trajectory: 1.5 fine steps per fine step


class MLMCConfig:
    """`MLMCConfig(steps, trajectories=None, tolerance=None, initial=2**14, min_levels=2, max_levels=10, seed=None,
    max_trajectories=2**28)`.  Level l runs steps·2^l steps; a payoff's Monitoring.every counts LEVEL-0 steps, so the
    contract dates are the same on every level.  Exactly one of
      trajectories=(N_0, …, N_L)  fixed levels and counts, no adaptivity — with a fixed seed, the reproducible form;
      tolerance=ε                 absolute, on the price: Giles' algorithm from `initial` trajectories on levels
                                  0 … min_levels, at most max_levels levels and max_trajectories trajectories in all.
    seed: None draws one; the seeds of batch b on level l are SeedSequence(seed, spawn_key=(l, b))."""

    def __init__(self, steps, trajectories=None, tolerance=None, initial=2 ** 14, min_levels=2, max_levels=10, seed=None,
                 max_trajectories=2 ** 28):
        self.steps = int(steps)
        if self.steps != steps or self.steps < 1:
            raise ValueError(f"MLMCConfig: steps must be a positive integer, not {steps!r}")
        if (trajectories is None) == (tolerance is None):
            raise ValueError("MLMCConfig: give exactly one of trajectories=(N_0, …, N_L) and tolerance=ε")
        self.initial, self.min_levels, self.max_levels = int(initial), int(min_levels), int(max_levels)
        self.max_trajectories = int(max_trajectories)
        self.trajectories, self.tolerance = None, None
        if trajectories is not None:
            self.trajectories = tuple(int(n) for n in trajectories)
            if not self.trajectories or any(n < 2 for n in self.trajectories):
                raise ValueError("MLMCConfig: trajectories is a non-empty sequence of counts >= 2 (a variance needs two)")
            top = len(self.trajectories) - 1
        else:
            self.tolerance = float(tolerance)
            if not (self.tolerance > 0.0 and math.isfinite(self.tolerance)):
                raise ValueError(f"MLMCConfig: tolerance must be positive and finite, not {tolerance!r}")
            if self.initial < 2:
                raise ValueError("MLMCConfig: initial must be at least 2 (a variance needs two)")
            if not 1 <= self.min_levels <= self.max_levels:
                raise ValueError("MLMCConfig: 1 <= min_levels <= max_levels")
            if self.max_trajectories < self.initial * (self.min_levels + 1):
                raise ValueError("MLMCConfig: max_trajectories must hold the initial trajectories of levels 0 … min_levels")
            top = self.max_levels
        if self.steps << top > MAX_STEPS:
            raise ValueError(f"MLMCConfig: the finest level would run {self.steps << top} steps (at most {MAX_STEPS})")
        self.seed = int(np.random.default_rng().integers(0, 2 ** 63)) if seed is None else int(seed)
        if self.seed < 0:
            raise ValueError("MLMCConfig: seed must not be negative")

    def level_steps(self, level):
        return self.steps << level

    def level_cost(self, level):
        """C_l, in steps per trajectory"""
        return float(self.level_steps(level)) * (1.0 if level == 0 else CORRECTION_COST)


def level_monitoring(every0, level):
    """monitor_every of level l for a Monitoring.every counted in level-0 steps"""
    return every0 << level


def level_seeds(seed, level, batch, n):
    """the seeds of batch b on level l: levels and batches are independent, a fixed seed gives fixed trajectories"""
    return np.random.SeedSequence(seed, spawn_key=(level, batch)).generate_state(n, np.uint64)


@dataclass(frozen=True)
class MultilevelMonteCarlo(AbstractPricingMethod):
    """The method of a multilevel solve; em_split / device as MonteCarlo's."""
    dynamics: Any
    strategy: Any
    config: MLMCConfig
    em_split: bool = True
    device: int = 0
    devices: Any = None  # refused: one device


@dataclass(frozen=True)
class MultilevelLevel:
    """steps of the level's fine grid; mean and variance of the discounted sample (P_0 on level 0, P_l − P_{l−1} above);
    fine_mean: the discounted mean of P_l itself"""
    steps: int
    trajectories: int
    mean: float
    variance: float
    fine_mean: float


@dataclass(frozen=True)
class MultilevelSolution:
    """price = Σ levels' means; std_error = √Σ(V_l/N_l); bias_estimate = max(|m_L|, |m_{L−1}|/2) (weak order 1 assumed;
    NaN without a correction); cost = Σ N_l·C_l in steps; converged: the tolerance form met both of its tests (always True
    in the fixed form, which has none)."""
    problem: Any
    method: Any
    price: float
    std_error: float
    levels: Any = field(default=())
    converged: bool = True
    bias_estimate: float = float("nan")
    cost: float = 0.0


class LevelSums:
    """Σ Y, Σ Y², Σ P_fine over the trajectories of a level so far (undiscounted), batch after batch"""

    def __init__(self):
        self.n, self.sum, self.sumsq, self.fine, self.batches = 0, 0.0, 0.0, 0.0, 0

    def add(self, n, s, ss, fine):
        self.n, self.sum, self.sumsq, self.fine, self.batches = self.n + n, self.sum + s, self.sumsq + ss, self.fine + fine, self.batches + 1

    def mean(self):
        return self.sum / self.n

    def variance(self):
        m = self.mean()
        v = (self.sumsq - self.n * m * m) / (self.n - 1.0) if self.n > 1 else 0.0
        return v if v > 0.0 else 0.0


def optimal_counts(tolerance, variances, costs):
    """N_l = ⌈2 ε⁻² √(V_l/C_l) Σ_k √(V_k C_k)⌉: the counts that bring Σ V_l/N_l to ε²/2 at the least Σ N_l C_l"""
    total = sum(math.sqrt(v * c) for v, c in zip(variances, costs))
    return [int(math.ceil(2.0 / (tolerance * tolerance) * math.sqrt(v / c) * total)) for v, c in zip(variances, costs)]


def bias_estimate(means):
    """max(|m_L|, |m_{L−1}|/2) over the corrections m_1 … m_L (means[0] is no correction): what is left beyond level L when
    the corrections halve per level — the weak order α = 1 of Euler–Maruyama, assumed, not fitted"""
    L = len(means) - 1
    if L < 1:
        return float("nan")
    b = abs(means[L])
    return max(b, abs(means[L - 1]) / 2.0) if L >= 2 else b


def drive(cfg: MLMCConfig, runner, discount=1.0):
    """The levels and counts of a solve.  runner(level, batch, n) -> (Σ Y, Σ Y², Σ P_fine) of n new trajectories.  Returns
    (LevelSums per level, converged)."""
    sums = []

    def top_up(level, target):
        while sums[level].n < target:
            n = min(BATCH, target - sums[level].n)
            sums[level].add(n, *runner(level, sums[level].batches, n))

    if cfg.trajectories is not None:
        for level, n in enumerate(cfg.trajectories):
            sums.append(LevelSums())
            top_up(level, n)
        return sums, True
    eps = cfg.tolerance
    targets = [cfg.initial] * (cfg.min_levels + 1)
    while True:
        while len(sums) < len(targets):
            sums.append(LevelSums())
        for level, n in enumerate(targets):
            top_up(level, n)
        costs = [cfg.level_cost(l) for l in range(len(sums))]
        want = optimal_counts(eps, [discount * discount * s.variance() for s in sums], costs)
        targets = [max(w, s.n) for w, s in zip(want, sums)]
        room = cfg.max_trajectories - sum(s.n for s in sums)
        short = [t - s.n for t, s in zip(targets, sums)]
        if sum(short) > room:  # run what the budget still holds, in level order, and stop
            for level, d in enumerate(short):
                take = min(d, room)
                top_up(level, sums[level].n + take)
                room -= take
            return sums, False
        if any(short):
            continue
        if bias_estimate([discount * s.mean() for s in sums]) <= eps / math.sqrt(2.0):
            return sums, True
        if len(sums) - 1 >= cfg.max_levels or cfg.max_trajectories - sum(s.n for s in sums) < cfg.initial:
            return sums, False
        targets.append(cfg.initial)


def check_supported(prob, method: MultilevelMonteCarlo, kw=None):
    """a MethodError that names what is supported, for everything else"""
    if kw:
        raise MethodError(f"MultilevelMonteCarlo draws its own noise and takes no {sorted(kw)}: {SUPPORTED}")
    if not isinstance(prob, PricingProblem):
        raise MethodError(f"a basket has no multilevel form: {SUPPORTED}")
    payoff, m, dyn, strat = prob.payoff, prob.market_inputs, method.dynamics, method.strategy
    if method.devices is not None:
        raise MethodError(f"MultilevelMonteCarlo does not shard over devices=: {SUPPORTED}")
    if isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, American):
        raise MethodError(f"American exercise is priced by LSM, which has no coupled levels: {SUPPORTED}")
    if isinstance(getattr(payoff, "monitoring", None), ContinuousMonitoring):
        raise MethodError(f"ContinuousMonitoring() needs the two levels' bridges coupled, which is not offered: {SUPPORTED}")
    vanilla = isinstance(payoff, VanillaOption) and isinstance(payoff.exercise_style, European) and isinstance(payoff.underlying, Spot)
    if not (vanilla or isinstance(payoff, PATH_PAYOFFS)):
        raise MethodError(f"{type(payoff).__name__}: {SUPPORTED}")
    ok = type(strat) is EulerMaruyama and (
        (isinstance(dyn, LognormalDynamics) and type(m) is BlackScholesInputs) or
        (isinstance(dyn, HestonDynamics) and type(m) is HestonInputs))
    if not ok:
        raise MethodError(f"no multilevel route for {type(dyn).__name__} + {type(strat).__name__} on {type(m).__name__}: "
                          f"{SUPPORTED}")
    if not isinstance(method.config, MLMCConfig):
        raise MethodError(f"MultilevelMonteCarlo takes an MLMCConfig, not a {type(method.config).__name__}: {SUPPORTED}")


def solve_mlmc(prob: PricingProblem, method: MultilevelMonteCarlo) -> MultilevelSolution:
    check_supported(prob, method)
    cfg, payoff = method.config, prob.payoff
    mon = path_monitoring(payoff, cfg.steps)  # ValueError when every does not divide the level-0 steps
    every0, start = mon if mon is not None else (cfg.steps, False)
    plain = MonteCarlo(method.dynamics, method.strategy, SimulationConfig(1, steps=cfg.steps, seeds=np.zeros(1, np.uint64)),
                       em_split=method.em_split, device=method.device)
    try:
        model, c, _, _, _ = _path_structs([payoff], prob.market_inputs, plain, routes().EULER)
        packed = (_ffi.hh_path_payoff * 1)(pack_path_payoff(payoff))
    except MethodError as e:  # a Dual in the inputs or in the payoff
        raise MethodError(f"{e}: {SUPPORTED}") from None
    ctx = _ffi.get_context(method.device)
    plain_entry = ctx.lib.hh_mc_solve_path_ex if isinstance(payoff, LookbackOption) else ctx.lib.hh_mc_solve_path
    mode = (_ffi.HH_EXTREMES_MONITORED,) if isinstance(payoff, LookbackOption) else ()

    def runner(level, batch, n):
        seeds = level_seeds(cfg.seed, level, batch, n)
        c.n_paths, c.n_steps = n, cfg.level_steps(level)
        c.seeds, c.seeds_on_device, c.seeds_len = seeds.ctypes.data, 0, n
        every = level_monitoring(every0, level)
        diff, fine = _ffi.hh_result(), _ffi.hh_result()
        if level == 0:
            ctx.check(plain_entry(ctx.handle, C.byref(model), C.byref(c), every, int(start), *mode, packed, 1, C.byref(diff),
                                  None, None))
            return diff.sum_payoff, diff.sumsq_payoff, diff.sum_payoff
        ctx.check(ctx.lib.hh_mc_solve_path_coupled(ctx.handle, C.byref(model), C.byref(c), every, int(start), packed, 1,
                                                   C.byref(diff), C.byref(fine), None, None))
        return diff.sum_payoff, diff.sumsq_payoff, fine.sum_payoff

    sums, converged = drive(cfg, runner, model.discount)
    return summarize(prob, method, sums, converged, model.discount)


def summarize(prob, method, sums, converged, discount):
    cfg = method.config
    levels = tuple(MultilevelLevel(cfg.level_steps(l), s.n, discount * s.mean(), discount * discount * s.variance(),
                                   discount * s.fine / s.n) for l, s in enumerate(sums))
    price = math.fsum(lv.mean for lv in levels)
    se = math.sqrt(math.fsum(lv.variance / lv.trajectories for lv in levels))
    cost = math.fsum(lv.trajectories * cfg.level_cost(l) for l, lv in enumerate(levels))
    return MultilevelSolution(prob, method, price, se, levels, converged, bias_estimate([lv.mean for lv in levels]), cost)
