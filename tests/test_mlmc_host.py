"""Multilevel Monte Carlo on the host side, without a GPU: the two entry points declared, exported and bound; every rule of
MLMCConfig; the step and monitoring schedule per level; the trajectory counts and the level-adding rule of the tolerance
form on hand-made variances and means (the per-level runner replaced by a stub); the seed derivation; every refusal of the
Python layer; the golden file against its maker and the margins it must show."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi, mlmc
from tests import mlmc_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_coupled": 8, "hh_mc_solve_path_coupled": 11}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------

def test_new_prototypes_are_declared_exported_and_bound():
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines()}
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None and name in exported
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6  # additions only
    section = text[text.index(" * Multilevel Monte Carlo (Giles 2008)"):text.index("int hh_mc_path_stats_coupled(")]
    for said in ("dW_c = dW_a + dW_b", "ANTITHETIC layout", "Two identities hold bit for bit", "HH_ERR_INVALID: n_steps odd",
                 "HH_ERR_UNSUPPORTED: antithetic", "Not provided: local volatility"):
        assert said in section, said


def test_solve_names_the_method_and_the_methods_are_distinct():
    assert "MultilevelMonteCarlo" in hh.solve.__doc__ and "MLMCConfig" in hh.solve.__doc__
    ml = hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.MLMCConfig(4, trajectories=(8, 8)))
    qm = hh.QuasiMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.SobolConfig(16, steps=4))
    plain = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(16, steps=4))
    assert not isinstance(qm, hh.MultilevelMonteCarlo) and not isinstance(plain, hh.MultilevelMonteCarlo)
    assert not isinstance(ml, (hh.QuasiMonteCarlo, hh.MonteCarlo))
    assert (ml.em_split, ml.device, ml.devices) == (True, 0, None)


# ---- MLMCConfig ------------------------------------------------------------------------------------------------------------

def test_config_rules():
    ok = hh.MLMCConfig(4, tolerance=0.05)
    assert (ok.steps, ok.trajectories, ok.tolerance, ok.initial, ok.min_levels, ok.max_levels, ok.max_trajectories) == \
        (4, None, 0.05, 2 ** 14, 2, 10, 2 ** 28)
    assert 0 <= ok.seed < 2 ** 63 and hh.MLMCConfig(4, tolerance=0.05).seed != ok.seed  # a drawn seed
    fixed = hh.MLMCConfig(4, trajectories=[100, 50, 25], seed=3)
    assert (fixed.trajectories, fixed.tolerance, fixed.seed) == ((100, 50, 25), None, 3)
    bad = [dict(steps=0, tolerance=0.1), dict(steps=2.5, tolerance=0.1), dict(steps=4),  # neither
           dict(steps=4, tolerance=0.1, trajectories=(8, 8)),  # both
           dict(steps=4, trajectories=()), dict(steps=4, trajectories=(8, 1)),
           dict(steps=4, tolerance=0.0), dict(steps=4, tolerance=-1.0), dict(steps=4, tolerance=math.inf),
           dict(steps=4, tolerance=math.nan), dict(steps=4, tolerance=0.1, initial=1),
           dict(steps=4, tolerance=0.1, min_levels=0), dict(steps=4, tolerance=0.1, min_levels=3, max_levels=2),
           dict(steps=4, tolerance=0.1, initial=100, min_levels=2, max_trajectories=299),
           dict(steps=4, tolerance=0.1, max_levels=16),          # 4·2^16 = 262144 steps > 262140
           dict(steps=2 ** 17, trajectories=(8, 8)),
           dict(steps=4, tolerance=0.1, seed=-1)]
    for kw in bad:
        with pytest.raises(ValueError, match="MLMCConfig"):
            hh.MLMCConfig(**kw)
    assert hh.MLMCConfig(4, tolerance=0.1, initial=100, min_levels=2, max_trajectories=300).max_trajectories == 300
    assert hh.MLMCConfig(4, tolerance=0.1, max_levels=15).level_steps(15) == 131072


def test_schedule_per_level():
    cfg = hh.MLMCConfig(4, trajectories=(8, 8, 8, 8))
    assert [cfg.level_steps(l) for l in range(4)] == [4, 8, 16, 32]
    assert [cfg.level_cost(l) for l in range(4)] == [4.0, 12.0, 24.0, 48.0]  # a correction: 1.5 fine steps per fine step
    # Monitoring.every counts level-0 steps: the dates stay where they are
    for every0 in (1, 2, 4):
        for l in range(4):
            every = mlmc.level_monitoring(every0, l)
            assert every == every0 * 2 ** l and cfg.level_steps(l) // every == 4 // every0
            assert l == 0 or (every % 2 == 0 and cfg.level_steps(l) % 2 == 0)  # what the coupled entry points ask for


def test_seed_derivation():
    a = mlmc.level_seeds(5, 2, 0, 1000)
    assert a.dtype == np.uint64 and a.shape == (1000,) and len(set(a.tolist())) == 1000
    np.testing.assert_array_equal(a, mlmc.level_seeds(5, 2, 0, 1000))
    np.testing.assert_array_equal(a, np.random.SeedSequence(5, spawn_key=(2, 0)).generate_state(1000, np.uint64))
    np.testing.assert_array_equal(a[:10], mlmc.level_seeds(5, 2, 0, 10))  # a shorter batch is a prefix
    for other in (mlmc.level_seeds(6, 2, 0, 1000), mlmc.level_seeds(5, 1, 0, 1000), mlmc.level_seeds(5, 2, 1, 1000),
                  mlmc.level_seeds(5, 0, 2, 1000)):
        assert not set(a.tolist()) & set(other.tolist())


# ---- the driver on a stub ----------------------------------------------------------------------------------------------------

class Stub:
    """a per-level runner whose trajectories so far always have exactly the mean m_l and the sample variance V_l"""

    def __init__(self, V, M):
        self.V, self.M, self.calls = V, M, []

    def __call__(self, level, batch, n):
        self.calls.append((level, batch, n))
        m, v = self.M[level], self.V[level]
        return n * m, (n - (batch == 0)) * v + n * m * m, n * (m + 1.0)


def test_optimal_counts_formula():
    V, Cst = [150.0, 12.0, 6.0], [4.0, 12.0, 24.0]
    eps = 0.05
    total = math.sqrt(600.0) + 12.0 + 12.0
    want = [math.ceil(2.0 / eps ** 2 * math.sqrt(v / c) * total) for v, c in zip(V, Cst)]
    got = mlmc.optimal_counts(eps, V, Cst)
    assert got == want and got[0] > got[1] > got[2]
    assert sum(v / n for v, n in zip(V, got)) <= eps ** 2 / 2.0  # what the counts are for
    assert sum(v / (n - 1) for v, n in zip(V, got)) > eps ** 2 / 2.0 * (1 - 1e-3)  # … and no more than that


def test_fixed_form_runs_what_it_is_told():
    stub = Stub([150.0, 12.0, 6.0], [7.0, 0.5, 0.25])
    sums, converged = mlmc.drive(hh.MLMCConfig(4, trajectories=(1000, 300, 100), seed=1), stub)
    assert converged and stub.calls == [(0, 0, 1000), (1, 0, 300), (2, 0, 100)]
    assert [s.n for s in sums] == [1000, 300, 100]
    assert [s.mean() for s in sums] == pytest.approx([7.0, 0.5, 0.25], rel=1e-14)
    assert [s.variance() for s in sums] == pytest.approx([150.0, 12.0, 6.0], rel=1e-12)
    assert [s.fine / s.n for s in sums] == pytest.approx([8.0, 1.5, 1.25], rel=1e-14)
    # more than one batch on a level: batch numbers count up
    big = Stub([1.0], [0.0])
    mlmc.drive(hh.MLMCConfig(4, trajectories=(2 * mlmc.BATCH + 5,), seed=1), big)
    assert big.calls == [(0, 0, mlmc.BATCH), (0, 1, mlmc.BATCH), (0, 2, 5)]


def test_tolerance_form_counts_and_levels():
    eps = 0.05
    V, M = [150.0, 12.0, 6.0, 3.0, 1.5, 0.75], [7.0, 0.2, 0.1, 0.05, 0.025, 0.0125]
    cfg = hh.MLMCConfig(4, tolerance=eps, initial=1000, seed=1)
    stub = Stub(V, M)
    sums, converged = mlmc.drive(cfg, stub)
    # levels are added while max(|m_L|, |m_{L−1}|/2) > ε/√2 = 0.03536: L = 2 (0.1), L = 3 (0.05), then L = 4 (0.025) stops
    assert converged and len(sums) == 5
    assert stub.calls[:3] == [(0, 0, 1000), (1, 0, 1000), (2, 0, 1000)]  # the initial trajectories on levels 0 … min_levels
    costs = [cfg.level_cost(l) for l in range(5)]
    assert [s.n for s in sums] == [max(1000, w) for w in mlmc.optimal_counts(eps, V[:5], costs)]
    assert sum(s.variance() / s.n for s in sums) <= eps ** 2 / 2.0 * (1 + 1e-9)
    # the rule itself
    assert math.isnan(mlmc.bias_estimate([7.0]))
    assert mlmc.bias_estimate([7.0, -0.2]) == 0.2                   # m_0 is no correction
    assert mlmc.bias_estimate([7.0, 0.2, -0.03]) == 0.1             # |m_1|/2 rules
    assert mlmc.bias_estimate([7.0, 0.2, 0.03, -0.04]) == 0.04
    # min_levels is honoured even where the corrections are already small
    small = Stub(V, [7.0, 0.001, 0.001, 0.001])
    sums, converged = mlmc.drive(hh.MLMCConfig(4, tolerance=eps, initial=1000, min_levels=3, seed=1), small)
    assert converged and len(sums) == 4
    # a discount scales means and tolerances alike: with D = 1/2 the corrections are halved and L = 3 is enough
    sums, converged = mlmc.drive(cfg, Stub(V, M), discount=0.5)
    assert converged and len(sums) == 4


def test_tolerance_form_gives_up_without_raising():
    eps = 0.05
    V, M = [150.0, 12.0, 6.0, 3.0, 1.5, 0.75], [7.0, 0.2, 0.2, 0.2, 0.2, 0.2]  # corrections that never shrink
    sums, converged = mlmc.drive(hh.MLMCConfig(4, tolerance=eps, initial=1000, max_levels=4, seed=1), Stub(V, M))
    assert not converged and len(sums) == 5
    # a budget that the optimal counts pass: what it holds is run, level by level, and the solve ends
    cfg = hh.MLMCConfig(4, tolerance=eps, initial=1000, max_trajectories=10_000, seed=1)
    sums, converged = mlmc.drive(cfg, Stub(V, M))
    assert not converged and sum(s.n for s in sums) == 10_000 and [s.n for s in sums][1:] == [1000, 1000]


# ---- the Python layer's refusals -------------------------------------------------------------------------------------------------

def heston(spot=100.0):
    return hh.HestonInputs(REF, 0.03, spot, 0.04, 1.5, 0.04, 0.3, -0.7)


def test_every_refusal_names_what_is_supported():
    cfg = hh.MLMCConfig(4, trajectories=(8, 8))
    ml = hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    call = hh.VanillaOption(100.0, EXP, hh.European(), hh.Call(), hh.Spot())
    bs = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    rows = [
        (hh.PricingProblem(call, heston()), hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, devices=range(2)), {}),
        (hh.PricingProblem(hh.VanillaOption(100.0, EXP, hh.American(), hh.Put(), hh.Spot()), heston()), ml, {}),
        (hh.PricingProblem(hh.VanillaOption(100.0, EXP, hh.European(), hh.Call(), hh.Forward()), heston()), ml, {}),
        (hh.PricingProblem(hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=hh.ContinuousMonitoring()), heston()), ml, {}),
        (hh.PricingProblem(hh.LookbackOption(EXP, hh.Call(), monitoring=hh.ContinuousMonitoring()), heston()), ml, {}),
        (hh.PricingProblem(call, heston(hh.Dual(100.0, (1.0,)))), ml, {}),
        (hh.PricingProblem(hh.AsianOption(hh.Dual(100.0, (1.0,)), EXP, hh.Call()), heston()), ml, {}),
        (hh.BasketPricingProblem([call, call], heston()), ml, {}),
        (hh.PricingProblem(call, heston()), ml, dict(ensemble=False)),
        (hh.PricingProblem(call, heston()), ml, dict(replay=np.zeros(4))),
        (hh.PricingProblem(call, bs), ml, {}),                                                      # model / dynamics mismatch
        (hh.PricingProblem(call, heston()), hh.MultilevelMonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg), {}),
        (hh.PricingProblem(call, heston()), hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.HestonBroadieKaya(), cfg), {}),
        (hh.PricingProblem(call, heston()), hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.HestonQE(), cfg), {}),
        (hh.PricingProblem(call, bs), hh.MultilevelMonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(), cfg), {}),
        (hh.PricingProblem(call, hh.MertonInputs(REF, 0.03, 100.0, 0.2, 0.5, -0.1, 0.2)),
         hh.MultilevelMonteCarlo(hh.MertonDynamics(), hh.EulerMaruyama(), cfg), {}),
        (hh.PricingProblem(call, heston()), hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(8, steps=4)), {}),
    ]
    for prob, method, kw in rows:
        with pytest.raises(hh.MethodError) as e:
            hh.solve(prob, method, **kw)
        assert mlmc.SUPPORTED in str(e.value), str(e.value)
    # a monitoring that does not divide the level-0 steps
    with pytest.raises(ValueError, match="divide"):
        hh.solve(hh.PricingProblem(hh.AsianOption(100.0, EXP, hh.Call(), None, hh.Monitoring(3)), heston()), ml)


# ---- the restatement and its golden file --------------------------------------------------------------------------------------

def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_file_is_what_its_maker_writes_and_keeps_its_margins():
    rec = mc.recorded()
    assert rec["steps"] == [4, 8, 16, 32] and rec["trajectories"] == list(mc.TRAJECTORIES) and rec["case"] == mc.MILD
    made = _load("tests/golden/make_mlmc_exact.py", "make_mlmc_exact").build()
    for seed in map(str, mc.RESTATED_SEEDS):
        for name in mc.PAYOFFS:
            got, want = rec["seeds"][seed][name], made["seeds"][seed][name]
            assert got["mean"] == pytest.approx(want["mean"], rel=1e-9) and got["var"] == pytest.approx(want["var"], rel=1e-9)
            V = got["var"]
            assert mc.MARGIN * V[1] <= mc.V1_OVER_VAR0 * V[0], (seed, name)
            for l in (1, 2):
                assert mc.MARGIN * V[l + 1] <= mc.DECAY * V[l], (seed, name, l, V[l + 1] / V[l])


def test_restated_coupling_is_exact_where_the_levels_coincide():
    """the restatement's own check: with σ = 0 and V0 = θ the variance is constant, the log-Euler step is exact in law and
    both legs end on the same spot up to rounding"""
    p = dict(mc.MILD, sigma=0.0)
    f, c = mc.coupled_stats(np.random.default_rng(3), 1000, 8, 2, p)
    np.testing.assert_allclose(f[mc.pc.S_T], c[mc.pc.S_T], rtol=1e-13)
    assert np.all(f[mc.pc.MAX_S] >= f[mc.pc.S_T]) and np.all(c[mc.pc.MIN_S] <= c[mc.pc.S_T])
