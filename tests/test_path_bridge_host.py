"""Continuous monitoring and lookbacks on the host side, without a GPU: the two entry points declared, exported and
bound; the row count of PathStatsLayout; how the new Python types are packed, grouped and refused; the payoff table on
hand-made statistics; the closed forms the device test prices against, held to an independent bridge simulation in
numpy; and the 50-digit restatement the device test uses, on the oracle's increments: every path usable for the chosen
seeds, bars of fp64 size, and a mirror that must swap its uniforms."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from hedgehog_jl_amd.basket import path_groups
from hedgehog_jl_amd.montecarlo import pack_path_payoff, path_extremes, path_monitoring
from tests import oracle_ffi
from tests.conftest import host_cxxflags, host_env
from tests import path_bridge_cases as bc
from tests import path_payoff_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_ex": 9, "hh_mc_solve_path_ex": 11}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
CONT = hh.ContinuousMonitoring()


def test_new_prototypes_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define HH_PATH_STATS 5\b", hdr) and re.search(r"#define HH_PATH_STATS_BRIDGE 7\b", hdr)
    for name, value in (("HH_EXTREMES_MONITORED", 0), ("HH_EXTREMES_BRIDGE", 1), ("HH_PAYOFF_LOOKBACK_FLOAT", 6),
                        ("HH_PAYOFF_LOOKBACK_FIXED", 7), ("HH_STAT_CMAX_S", 5), ("HH_STAT_CMIN_S", 6)):
        assert re.search(name + r"\s*=\s*%d\b" % value, hdr), name
        assert getattr(_ffi, name) == value
    assert (_ffi.HH_PATH_STATS, _ffi.HH_PATH_STATS_BRIDGE) == (5, 7)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_layout_has_five_or_seven_rows(tmp_path):
    src = ['#include <cstdio>', f'#include "{os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_layout.h")}"', "int main() {",
           "  const hh::PathStatsLayout a(10, false), b(10, true), c(10, true, HH_PATH_STATS_BRIDGE), d(3, false, HH_PATH_STATS);",
           '  std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", a.total, b.total, c.total, d.total, c.n_total, c.row(HH_STAT_CMAX_S),',
           "              c.row(HH_STAT_CMIN_S), b.row(HH_STAT_S_T));", "  return 0;", "}"]
    (tmp_path / "probe.cpp").write_text("\n".join(src))
    subprocess.run(["g++", *host_cxxflags(), "-std=c++17", "-Wall", "-Werror", str(tmp_path / "probe.cpp"), "-o",
                    str(tmp_path / "probe")], check=True)  # (the sanitizer build of the host checks, when that is asked for)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True, env=host_env()).stdout.split()
    assert [int(t) for t in out] == [50, 100, 140, 15, 20, 100, 120, 80]


def fields(q):
    return (q.kind, q.barrier_type, q.strike, q.cp, q.barrier, q.rebate, q.cash)


def test_the_new_types_are_packed_and_say_their_extremes():
    m3 = hh.Monitoring(3, True)
    assert fields(pack_path_payoff(hh.LookbackOption(EXP, hh.Call()))) == (bc.LB_FLOAT, 0, 0.0, 1.0, 0.0, 0.0, 0.0)
    assert fields(pack_path_payoff(hh.LookbackOption(EXP, hh.Put(), monitoring=CONT))) == (bc.LB_FLOAT, 0, 0.0, -1.0, 0.0, 0.0, 0.0)
    assert fields(pack_path_payoff(hh.LookbackOption(EXP, hh.Put(), 95.0, m3))) == (bc.LB_FIXED, 0, 95.0, -1.0, 0.0, 0.0, 0.0)
    assert fields(pack_path_payoff(hh.LookbackOption(EXP, hh.Call(), strike=0.0))) == (bc.LB_FIXED, 0, 0.0, 1.0, 0.0, 0.0, 0.0)
    b = hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndIn(), rebate=2.5, monitoring=CONT)
    assert fields(pack_path_payoff(b)) == (pc.BARRIER, pc.UP_IN, 100.0, 1.0, 120.0, 2.5, 0.0)
    assert b.monitoring == hh.ContinuousMonitoring() and repr(b.monitoring) == "ContinuousMonitoring()"
    # a continuous payoff has no dates of its own, as a digital has none
    assert path_monitoring(b, 12) is None and path_monitoring(hh.LookbackOption(EXP, hh.Call(), monitoring=CONT), 7) is None
    assert path_monitoring(hh.LookbackOption(EXP, hh.Call(), monitoring=m3), 12) == (3, True)
    assert hh.LookbackOption(EXP, hh.Call()).monitoring == hh.Monitoring(1, False)
    assert path_extremes(b) == bc.BRIDGE and path_extremes(hh.LookbackOption(EXP, hh.Call())) == bc.MONITORED
    assert path_extremes(hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndIn())) == bc.MONITORED
    assert path_extremes(hh.AsianOption(100.0, EXP, hh.Call())) is None and path_extremes(hh.DigitalOption(1.0, EXP, hh.Call())) is None
    for wrong in (hh.ArithmeticAverage(), 3, "continuous", hh.ContinuousMonitoring):
        with pytest.raises(TypeError, match="monitoring"):
            hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=wrong)
        with pytest.raises(TypeError, match="monitoring"):
            hh.LookbackOption(EXP, hh.Call(), monitoring=wrong)
    with pytest.raises(TypeError, match="monitoring"):  # an average over a continuum is not offered
        hh.AsianOption(100.0, EXP, hh.Call(), None, CONT)
    with pytest.raises(TypeError, match="call_put"):
        hh.LookbackOption(EXP, hh.European())


def heston(spot=100.0):
    return hh.HestonInputs(REF, 0.03, spot, 0.04, 2.0, 0.04, 0.3, -0.7)


def test_unsupported_combinations_raise_before_any_device_work():
    cfg = hh.SimulationConfig(100, steps=12)
    payoffs = [hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=CONT),
               hh.LookbackOption(EXP, hh.Call(), monitoring=CONT), hh.LookbackOption(EXP, hh.Put(), 100.0, hh.Monitoring(3))]
    euler_h = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    bs = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    for payoff in payoffs:
        with pytest.raises(hh.MethodError, match="FiniteDifference"):
            hh.solve(hh.PricingProblem(payoff, heston(hh.Dual(100.0, (1.0,)))), euler_h)
        with pytest.raises(hh.MethodError, match="FiniteDifference"):
            hh.solve(hh.GreekProblem(hh.PricingProblem(payoff, heston()), hh.SpotLens()), hh.ForwardAD(), euler_h)
        with pytest.raises(hh.MethodError, match="EulerMaruyama"):
            hh.solve(hh.PricingProblem(payoff, bs), hh.MonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(), cfg))
        with pytest.raises(hh.MethodError, match="EulerMaruyama"):
            hh.solve(hh.PricingProblem(payoff, heston()), hh.MonteCarlo(hh.HestonDynamics(), hh.HestonBroadieKaya(), cfg))
        with pytest.raises(hh.MethodError):
            hh.solve(hh.PricingProblem(payoff, bs), euler_h)
        with pytest.raises(hh.MethodError, match="devices"):
            hh.solve(hh.PricingProblem(payoff, heston()), hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, devices=range(2)))
        assert hh.solve_montecarlo_many([hh.PricingProblem(payoff, heston(101.0)), hh.PricingProblem(payoff, heston(99.0))], euler_h) is None
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.PricingProblem(hh.LookbackOption(EXP, hh.Call(), hh.Dual(100.0, (1.0,)), CONT), heston()), euler_h)
    with pytest.raises(ValueError, match="divide"):
        hh.solve(hh.PricingProblem(hh.LookbackOption(EXP, hh.Call(), monitoring=hh.Monitoring(5)), heston()), euler_h)
    # one call has one extremes mode
    from hedgehog_jl_amd.montecarlo import solve_path_payoffs
    with pytest.raises(ValueError, match="extremes mode"):
        solve_path_payoffs([payoffs[0], hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=hh.Monitoring(12))],
                           heston(), euler_h)


def test_basket_grouping_by_extremes_mode():
    ticks = hh.to_ticks(EXP)
    m1, m3 = hh.Monitoring(1), hh.Monitoring(3)
    asian = hh.AsianOption(100.0, EXP, hh.Call(), None, m1)
    cont = hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=CONT)
    disc = hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=m1)
    digital = hh.DigitalOption(100.0, EXP, hh.Call())
    look = hh.LookbackOption(EXP, hh.Call(), monitoring=CONT)
    look3 = hh.LookbackOption(EXP, hh.Put(), 100.0, m3)
    # a daily Asian, a continuous barrier and a digital: one simulation
    assert path_groups([asian, cont, digital], 12) == [((ticks, (1, False)), [0, 1, 2])]
    # a discrete and a continuous barrier: two
    assert path_groups([disc, cont], 12) == [((ticks, (1, False)), [0]), ((ticks, None), [1])]
    # the Asian shares the discrete barrier's group, so the continuous payoffs stand alone, with nobody's dates
    assert path_groups([asian, disc, cont, look, digital], 12) == [((ticks, (1, False)), [0, 1, 4]), ((ticks, None), [2, 3])]
    # continuous payoffs alone take the digital along; a monitored lookback groups by its dates
    assert path_groups([cont, digital, look3, look], 12) == [((ticks, (3, False)), [1, 2]), ((ticks, None), [0, 3])]
    later = hh.LookbackOption(hh.Date(2023, 1, 1), hh.Call(), monitoring=CONT)
    assert path_groups([asian, later], 12) == [((ticks, (1, False)), [0]), ((hh.to_ticks(hh.Date(2023, 1, 1)), None), [1])]


def test_payoff_table_on_hand_made_statistics():
    #                 path:   0      1      2
    stats = np.array([[300.0, 330.0, 270.0], [13.8, 14.1, 13.5],
                      [105.0, 120.0, 100.0], [95.0, 100.0, 80.0],      # MAX_S, MIN_S on the dates
                      [100.0, 115.0, 85.0],                            # S_T
                      [107.0, 121.0, 100.5], [94.0, 99.0, 79.0]])      # CMAX_S, CMIN_S
    f = lambda q, e: bc.payoff_from_stats(stats, q, 3, e).tolist()  # noqa: E731
    assert f(pc.payoff(bc.LB_FLOAT, cp=1.0), bc.MONITORED) == [5.0, 15.0, 5.0]
    assert f(pc.payoff(bc.LB_FLOAT, cp=1.0), bc.BRIDGE) == [6.0, 16.0, 6.0]
    assert f(pc.payoff(bc.LB_FLOAT, cp=-1.0), bc.MONITORED) == [5.0, 5.0, 15.0]
    assert f(pc.payoff(bc.LB_FLOAT, cp=-1.0), bc.BRIDGE) == [7.0, 6.0, 15.5]
    assert f(pc.payoff(bc.LB_FIXED, 104.0, 1.0), bc.MONITORED) == [1.0, 16.0, 0.0]
    assert f(pc.payoff(bc.LB_FIXED, 104.0, 1.0), bc.BRIDGE) == [3.0, 17.0, 0.0]
    assert f(pc.payoff(bc.LB_FIXED, 96.0, -1.0), bc.MONITORED) == [1.0, 0.0, 16.0]
    assert f(pc.payoff(bc.LB_FIXED, 96.0, -1.0), bc.BRIDGE) == [2.0, 0.0, 17.0]
    # a barrier between the discrete and the continuous maximum is hit under the bridge only; a touch counts
    up = pc.payoff(pc.BARRIER, 90.0, 1.0, pc.UP_OUT, 107.0, 1.5)
    assert f(up, bc.MONITORED) == [10.0, 1.5, 0.0] and f(up, bc.BRIDGE) == [1.5, 1.5, 0.0]
    down = pc.payoff(pc.BARRIER, 90.0, 1.0, pc.DOWN_IN, 94.5, 1.5)
    assert f(down, bc.MONITORED) == [1.5, 1.5, 0.0] and f(down, bc.BRIDGE) == [10.0, 1.5, 0.0]
    # kinds that read no extremes are the same under both
    for q in (pc.payoff(pc.ARITH, 100.0, 1.0), pc.payoff(pc.GEOM, 95.0, -1.0), pc.payoff(pc.DCASH, 100.0, 1.0, cash=2.0),
              pc.payoff(pc.DASSET, 100.0, -1.0), pc.payoff(pc.VANILLA, 99.0, 1.0)):
        assert f(q, bc.MONITORED) == f(q, bc.BRIDGE) == pc.payoff_from_stats(stats[:5], q, 3).tolist()


def test_closed_forms_against_an_independent_bridge_simulation():
    """2^18 exact lognormal paths on 16 dates (numpy's generator, nothing of the library), the extremes of every step by
    the bridge's inverted laws: both closed forms within 4 standard errors, in/out parity in the formulas, and the
    discretely monitored prices at least 10 standard errors away — what the device test asserts of the kernels."""
    S0, K, B, r, sigma, T, steps, n = 100.0, 100.0, 120.0, 0.05, 0.2, 1.0, 16, 2**18
    dt, D = T / steps, math.exp(-r * T)
    rng = np.random.default_rng(7)
    x = math.log(S0) + np.cumsum((r - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * rng.standard_normal((steps, n)), axis=0)
    x = np.vstack([np.full((1, n), math.log(S0)), x])
    L1, L2 = -2.0 * np.log(rng.random((steps, n))), -2.0 * np.log(rng.random((steps, n)))
    d2, mid = (x[1:] - x[:-1]) ** 2, x[1:] + x[:-1]
    cmax = np.exp(np.maximum(0.5 * (mid + np.sqrt(d2 + sigma * sigma * dt * L1)).max(axis=0), x.max(axis=0)))
    cmin = np.exp(np.minimum(0.5 * (mid - np.sqrt(d2 + sigma * sigma * dt * L2)).min(axis=0), x.min(axis=0)))
    S_T, dmax, dmin = np.exp(x[-1]), np.exp(x.max(axis=0)), np.exp(x.min(axis=0))
    van = np.maximum(S_T - K, 0.0)
    exact_uo, exact_lb = bc.up_and_out_call(S0, K, B, r, sigma, T), bc.floating_lookback_call(S0, r, sigma, T)
    assert exact_uo == pytest.approx(1.176, abs=2e-3)  # the issue's figure
    for what, cont, disc, exact in (("up-and-out", np.where(cmax >= B, 0.0, van), np.where(dmax >= B, 0.0, van), exact_uo),
                                    ("lookback", S_T - cmin, S_T - dmin, exact_lb)):
        z = [(D * p.mean() - exact) / (D * p.std(ddof=1) / math.sqrt(n)) for p in (cont, disc)]
        print(f"\n{what}: exact {exact:.6f} bridge z {z[0]:+.2f} monitored z {z[1]:+.2f}")
        assert abs(z[0]) <= 4.0 and abs(z[1]) >= 10.0, (what, z)
    # a barrier out of reach is the vanilla; a barrier at the spot leaves nothing
    assert bc.up_and_out_call(S0, K, 1e6, r, sigma, T) == pytest.approx(bc.bs_call(S0, K, r, sigma, T), rel=1e-9)
    assert bc.up_and_out_call(S0, K, S0 * (1 + 1e-12), r, sigma, T) == pytest.approx(0.0, abs=1e-8)


@pytest.fixture(scope="module")
def oracle():
    return oracle_ffi.load()


def test_bridge_uniforms_are_those_of_the_oracles_philox(oracle):
    seeds = bc.live_seeds("lognormal")[:3]
    U = bc.bridge_uniforms(oracle, seeds, 4)
    assert U.shape == (3, 4, 2) and np.all((U > 0.0) & (U < 1.0)) and len(np.unique(U)) == U.size
    c = oracle.philox([2, 0, 0, 3], [int(seeds[1]) & 0xFFFFFFFF, int(seeds[1]) >> 32])
    assert U[1, 2, 0] == ((((int(c[1]) << 32) | int(c[0])) >> 12) + 0.5) * 2.0 ** -52
    # another domain than the Euler increments': the block of counter (k, 0, 0, 0) is not this one
    assert not np.array_equal(c, oracle.philox([2, 0, 0, 0], [int(seeds[1]) & 0xFFFFFFFF, int(seeds[1]) >> 32]))


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(bc.LIVE))
def test_restatement_on_the_oracles_increments(oracle, name, anti):
    """The reference alone, on the seeds the device test uses: every path usable (at most 2 % may be left out: none of
    32), the clipped case clipped, the bars of fp64 size, the extremes ordered, and — antithetic — the mirror's maximum
    taken with the unswapped uniform outside its bar on most paths, so the device test discriminates."""
    model, dyn, split, steps, _ = bc.LIVE[name]
    seeds = bc.live_seeds(name)
    heston_dyn = dyn == "heston"
    tiled = oracle.wiener_fill(_ffi.HH_HESTON if heston_dyn else _ffi.HH_LOGNORMAL, model["rho"], model["T"], steps, seeds)
    case = bc.live_case(name, anti, bc.increments_of(tiled, bc.N_LIVE, steps, 2 if heston_dyn else 1))
    ref = bc.reference(case, bc.bridge_uniforms(oracle, seeds, steps))
    left_out = bc.N_LIVE - int(ref["usable"].sum())
    print(f"\n{name} antithetic={anti}: {left_out} of {bc.N_LIVE} left out, clip fraction {ref['clip_fraction']:.3f}")
    assert left_out <= bc.MAX_UNUSABLE * bc.N_LIVE
    if name == "heston-classic-clipped":
        assert ref["clip_fraction"] >= bc.MIN_CLIP_FRACTION
    bars = bc.bar(ref["e64"], ref["A"])
    for m in range(ref["members"]):
        want = np.array([[float(t) for t in row] for row in ref["want"][m]])
        assert np.all(want[:, 1] >= want[:, 0]) and np.all(want[:, 2] <= want[:, 0])      # CMAX_S >= S_T >= CMIN_S
        assert np.all(want[:, 1] >= model["S0"] * (1 - 1e-15)) and np.all(want[:, 2] <= model["S0"] * (1 + 1e-15))
        assert np.all(bars[m] <= 1e-10 * want), (name, float(np.max(bars[m] / want)))  # some thousand ulp at the most
        assert np.all(ref["e64"][m] <= bars[m])
    if anti:
        wrong = np.array([float(abs(w - t[1])) for w, t in zip(ref["wrong_cmax"], ref["want"][1])])
        assert (wrong > bars[1][:, 1]).mean() > 0.5
