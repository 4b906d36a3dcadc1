"""Pathwise derivatives of the path payoffs on the host side, without a GPU: the inputs of the device test (usable paths,
clipped steps, strikes with paths on both sides), the size of its bars, the 50-digit restatement's tangent rows held to
central differences of its OWN walk, the three entry points declared, exported and bound, and every refusal of
Pathwise() in its own words beside ForwardAD's unchanged one."""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex
from tests import euler_tangent_cases as tc
from tests import oracle_ffi
from tests import path_tangent_cases as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_tangent": 9, "hh_mc_solve_path_tangent": 9}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


@pytest.fixture(scope="module")
def oracle():
    return oracle_ffi.load()


def cases_of(oracle, name):
    for shape in tg.SHAPES:
        dW = tg.increments(oracle, name, shape[0])
        for start in (0, 1):
            for anti in (0, 1):
                yield tg.case_of(name, shape, start, anti, dW)


# ---- the inputs of the device test -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tg.MODELS))
def test_the_reference_keeps_all_but_one_path_and_the_strikes_split_them(oracle, name):
    """On the oracle's increments of seeds_of(name): at most MAX_UNUSABLE of a case's 65 paths unusable for any payoff, the
    clipped model clipped on the shapes that have a second step, the bars fp64-sized (euler_tangent_cases' rule and
    limit), and — without the mirror, where a sample is one member's payoff — every kind with a strike in the money on
    some paths and out of it on others."""
    for case in cases_of(oracle, name):
        ref = tg.reference(case)
        n = ref["n"]
        assert n == tg.N_PATHS
        for pj in ref["payoffs"]:
            assert n - int(pj["usable"].sum()) <= tg.MAX_UNUSABLE * n, case["id"]
        assert n - int(ref["usable_all"].sum()) <= tg.MAX_UNUSABLE * n, case["id"]
        if name == "heston-classic-clipped" and case["n_steps"] > 1:
            assert ref["clip_fraction"] >= tg.MIN_CLIP_FRACTION, case["id"]
        # (one date: the floating lookback is S_T − S_T, an exact zero whose terms have magnitudes — the rule sizes bars
        # against values and has none here; the device test holds it to == 0)
        sized = ref if tg.n_mon_of(case) > 1 else dict(ref, payoffs=[pj for k, pj in zip(case["kinds"], ref["payoffs"])
                                                                      if k != tg.LB_FLOAT])
        tc.assert_bars_are_fp64_sized(sized, int(case["antithetic"]), 1e-9)
        if not case["antithetic"]:
            for kind, pj in zip(case["kinds"], ref["payoffs"]):
                if kind != tg.LB_FLOAT:
                    itm = sum(1 for row in pj["payoff"] if row[0] > 0)
                    assert 5 <= itm <= n - 5, (case["id"], kind, pj["strike"], pj["cp"])
        # the statistics' own bars: every value row within 1e-10 of its value
        for stat in tg.STATS:
            st = ref["stat"][stat]
            bars = tc.path_bar(st["e64"], st["A"])[..., 0]
            vals = np.array([[abs(float(row[0])) for row in mem] for mem in st["want"]])
            assert np.all(bars <= 1e-10 * np.maximum(vals, 1.0)), (case["id"], stat)


# ---- the rules, with no device in it -----------------------------------------------------------------------------------

BUMP = mp.mpf(10) ** -20
CD_CASES = (("lognormal", (5, 1), 1, 1), ("heston-split", (6, 3), 0, 1), ("heston-classic", (5, 1), 1, 0),
            ("heston-classic-clipped", (5, 1), 1, 1))


@pytest.mark.parametrize("name,shape,start,anti", CD_CASES)
def test_tangent_rows_are_central_differences_of_the_walk(oracle, name, shape, start, anti):
    """Each of the eight slots bumped by ±1e-20 of its value in the restatement's own 50-digit walk: the central difference
    of every statistic of every member and of every payoff equals the Dual's partial to 1e-15 of its scale (the
    truncation is 1e-40, the rounding 1e-30), on usable paths — where every comparison has a margin of 2⁻³⁰ of its
    magnitude, which no such bump crosses."""
    dW = tg.increments(oracle, name, shape[0])[:8]
    case = tg.case_of(name, shape, start, anti, dW)
    ref = tg.reference(case)
    members, usable = ref["members"], np.flatnonzero(ref["usable_all"])
    assert len(usable) >= 6
    with mp.workdps(ex.DPS):
        for s, slot in enumerate(tg.SLOTS):
            sides = []
            for sign in (1, -1):
                b = dict(case, rows={})
                payoffs = list(case["payoff_list"])
                if slot == "strike":
                    payoffs = [(mp.mpf(K) * (1 + sign * BUMP), cp) for K, cp in payoffs]
                    h = None
                else:
                    b[slot] = mp.mpf(case[slot]) * (1 + sign * BUMP)
                    b["walk_key"] = case["walk_key"] + (slot, sign)
                sides.append((tg.run(b, mp.mpf, payoffs), b["rows"]["mp"]))
            (up, up_rows), (dn, dn_rows) = sides
            for i in usable:
                if slot != "strike":
                    h = 2 * mp.mpf(case[slot]) * BUMP
                    for m in range(members):
                        for stat in tg.STATS + ("SUM_KS",):
                            cd = (up_rows[i][m][stat].v - dn_rows[i][m][stat].v) / h
                            want = ref["stat"][stat]["want"][m][i]
                            assert abs(cd - want[1 + s]) <= mp.mpf(10) ** -15 * max(1, abs(want[0]), abs(want[1 + s])), \
                                (slot, stat, i, m)
                        assert up_rows[i][m]["K_MAX"] == ref["k_max"][m][i] and up_rows[i][m]["K_MIN"] == ref["k_min"][m][i]
                for j, pj in enumerate(ref["payoffs"]):
                    K = mp.mpf(pj["strike"])
                    hj = 2 * K * BUMP if slot == "strike" else h
                    if hj == 0:  # the floating lookback's strike is 0 and not read
                        assert pj["payoff"][i][1 + s] == 0
                        continue
                    for what in ("payoff", "price"):
                        cd = (up[i]["payoffs"][j][what].v - dn[i]["payoffs"][j][what].v) / hj
                        want = pj[what][i]
                        assert abs(cd - want[1 + s]) <= mp.mpf(10) ** -15 * max(1, abs(want[0]), abs(want[1 + s])), \
                            (slot, what, j, i)


def test_the_tie_rule_keeps_the_first_date():
    """equal spots on two dates (zero increments, zero drift): the extreme stays with the first one"""
    model = dict(tg.H, sigma=0.0, r_drift=0.0)
    case = dict(model, id="tie", walk_key=("tie",), dynamics="lognormal", em_split=1, n_steps=3, monitor_every=1,
                include_start=1, antithetic=0, dW=np.zeros((1, 3, 1)), kinds=[tg.LB_FLOAT], payoff_list=[(0.0, 1.0)], rows={})
    with mp.workdps(ex.DPS):
        tg.run(case, mp.mpf, case["payoff_list"])
    st = case["rows"]["mp"][0][0]
    assert (st["K_MAX"], st["K_MIN"]) == (0, 0) and st["MAX_S"].v == st["MIN_S"].v == st["S_T"].v


# ---- the ABI's declarations --------------------------------------------------------------------------------------------

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
    assert re.search(r"\bsize_t\s+hh_path_tangent_rows\s*\(\s*uint32_t\s+n_active\s*\)\s*;", hdr)
    assert bound["hh_path_tangent_rows"][1] is C.c_size_t and bound["hh_path_tangent_rows"][2] == [C.c_uint32]
    assert [lib.hh_path_tangent_rows(n) for n in range(5)] == [8, 13, 18, 23, 28]
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    for name, value in (("HH_TANGENT_DATE_ROWS", 3), ("HH_TANGENT_ROWS_PER_SLOT", 5), ("HH_TANGENT_MAX_BASIS", 4)):
        assert re.search(rf"#define {name} {value}\b", hdr) and getattr(_ffi, name) == value
    enums = dict(re.findall(r"\b(HH_(?:TANGENT|BASIS)_[A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert len(enums) == 12
    for name, value in enums.items():
        assert getattr(_ffi, name) == int(value), name
    assert (_ffi.HH_TANGENT_K_MAX, _ffi.HH_TANGENT_K_MIN, _ffi.HH_TANGENT_SUM_KS) == (5, 6, 7)
    assert (_ffi.HH_TANGENT_DSUM_S, _ffi.HH_TANGENT_DSUM_X, _ffi.HH_TANGENT_DMAX_S, _ffi.HH_TANGENT_DMIN_S,
            _ffi.HH_TANGENT_DS_T) == (_ffi.HH_STAT_SUM_S, _ffi.HH_STAT_SUM_X, _ffi.HH_STAT_MAX_S, _ffi.HH_STAT_MIN_S,
                                      _ffi.HH_STAT_S_T)


# ---- Python: what Pathwise() refuses, and what stays ------------------------------------------------------------------

def heston(**kw):
    args = dict(spot=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7)
    args.update(kw)
    return hh.HestonInputs(REF, 0.03, args["spot"], args["V0"], args["kappa"], args["theta"], args["sigma"], args["rho"])


def test_pathwise_refusals_and_the_unchanged_forward_ad_error():
    cfg = hh.SimulationConfig(64, steps=12)
    mon = hh.Monitoring(3, True)
    asian = hh.AsianOption(100.0, EXP, hh.Call(), hh.ArithmeticAverage(), mon)
    euler = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    spot, pw = hh.SpotLens(), hh.Pathwise()

    def greek(payoff, method, lens=spot, inputs=None, **kw):
        return hh.solve(hh.GreekProblem(hh.PricingProblem(payoff, inputs or heston()), lens), pw, method, **kw)

    assert issubclass(hh.Pathwise, hh.greeks.GreekMethod) and hh.Pathwise is hh.greeks.Pathwise
    for payoff in (hh.BarrierOption(100.0, 120.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=mon),
                   hh.DigitalOption(100.0, EXP, hh.Call())):
        with pytest.raises(hh.MethodError, match="discontinuous payoff omits the jump term — use FiniteDifference"):
            greek(payoff, euler)
        with pytest.raises(hh.MethodError, match="discontinuous"):
            hh.solve(hh.BatchGreekProblem(hh.PricingProblem(payoff, heston()), (spot,)), pw, euler)
    with pytest.raises(hh.MethodError, match=r"not offered under ContinuousMonitoring\(\)"):
        greek(hh.LookbackOption(EXP, hh.Call(), None, hh.ContinuousMonitoring()), euler)
    with pytest.raises(hh.MethodError, match="plain Euler route .* not on HestonQE"):
        greek(asian, hh.MonteCarlo(hh.HestonDynamics(), hh.HestonQE(), cfg))
    with pytest.raises(hh.MethodError, match="plain Euler route .* HestonBroadieKaya"):
        greek(asian, hh.MonteCarlo(hh.HestonDynamics(), hh.HestonBroadieKaya(), cfg))
    with pytest.raises(hh.MethodError, match="plain Euler route .* not on Merton paths"):
        greek(asian, hh.MonteCarlo(hh.MertonDynamics(), hh.EulerMaruyama(), cfg),
              inputs=hh.MertonInputs(REF, 0.03, 100.0, 0.2, 0.5, -0.1, 0.15))
    with pytest.raises(hh.MethodError, match="runs on one device"):
        greek(asian, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, devices=range(2)))
    with pytest.raises(hh.MethodError, match="no replay"):
        greek(asian, euler, replay=np.zeros((64, 12, 2)))
    with pytest.raises(hh.MethodError, match="not CarrMadan"):
        greek(asian, hh.CarrMadan(1.0, 32.0, hh.HestonDynamics()))
    with pytest.raises(hh.MethodError, match="1 .. 8 lenses"):
        hh.solve(hh.BatchGreekProblem(hh.PricingProblem(asian, heston()), (spot,) * 9), pw, euler)
    with pytest.raises(hh.MethodError, match="ρ is not supported"):  # the MethodError it is on ForwardAD's plain route
        greek(asian, euler, lens=hh.optic("market_inputs.ρ"))
    # ForwardAD on a path payoff, and a Dual handed to solve: today's words, verbatim
    words = "path-dependent payoffs carry no dual partials: use FiniteDifference"
    with pytest.raises(hh.MethodError) as e:
        hh.solve(hh.GreekProblem(hh.PricingProblem(asian, heston()), spot), hh.ForwardAD(), euler)
    assert str(e.value) == words
    with pytest.raises(hh.MethodError) as e:
        hh.solve(hh.PricingProblem(asian, heston(spot=hh.Dual(100.0, (1.0,)))), euler)
    assert str(e.value) == words
