"""Continuous barriers and lookbacks by Brownian bridge on the device (hh_mc_path_stats_ex, hh_mc_solve_path_ex; the
bridge form of path_stats_kernel, csrc/hh_path.hip).

(1) nothing that existed moved; (2) the continuous extremes against a 50-digit restatement on live increments; (3) they
bound the discrete ones; (4) the closed forms of continuous monitoring under lognormal dynamics, which the monitored
mode misses; (5) per-path identities and independence of what else is in a call; (6) the argument errors; (7) the Python
layer.  Shapes and models are tests/test_gpu_path_payoff.py's, for its reasons."""
import ctypes as C
import math

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import oracle_ffi
from tests import path_bridge_cases as bc
from tests import path_payoff_cases as pc
from tests import test_gpu_path_payoff as base

pytestmark = pytest.mark.gpu

LOGN, HEST, EULER = base.LOGN, base.HEST, base.EULER
INV, UNS = base.INV, base.UNS
MODELS, SHAPES, U = base.MODELS, base.SHAPES, base.U
MONITORED, BRIDGE = bc.MONITORED, bc.BRIDGE
config, n_total, seeds_for = base.config, base.n_total, base.seeds_for


def path_stats_ex(ctx, m, c, every, start, extremes):
    stats = np.empty((bc.ROWS[extremes], n_total(c)))
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_ex(ctx.handle, C.byref(m), C.byref(c), every, start, extremes, stats.ctypes.data, 0,
                                          C.byref(res)))
    assert res.n_paths_done == c.n_paths and res.kernel_ms > 0.0
    return stats


def solve_path_ex(ctx, m, c, every, start, extremes, payoffs):
    """-> (results, per-member payoffs (K, n_total), statistics (5 or 7, n_total))"""
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = np.empty((K, n_total(c))), np.empty((bc.ROWS[extremes], n_total(c)))
    ctx.check(ctx.lib.hh_mc_solve_path_ex(ctx.handle, C.byref(m), C.byref(c), every, start, extremes, arr, K, res,
                                          values.ctypes.data, stats.ctypes.data))
    return list(res), values, stats


def key(r):
    return (r.price, r.std_error, r.sum_payoff, r.sumsq_payoff, r.n_paths_done, tuple(r.dprice))


# ---- (1) nothing moved -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(MODELS))
def test_the_five_statistics_are_unchanged(hhlib, name, anti):
    dyn, split, params = MODELS[name]
    m = _ffi.make_model(**params)
    for n, steps, every, start in SHAPES:
        c = config(dyn, n, steps, anti, split)
        five = base.path_stats(hhlib, m, c, every, start)
        seven = path_stats_ex(hhlib, m, c, every, start, BRIDGE)
        where = str((name, anti, n, steps, every, start))
        np.testing.assert_array_equal(seven[:5], five, err_msg=where)
        np.testing.assert_array_equal(path_stats_ex(hhlib, m, c, every, start, MONITORED), five, err_msg=where)
        assert np.all(np.isfinite(seven)) and np.all(seven[bc.CMIN_S] > 0.0), where


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(MODELS))
def test_monitored_mode_is_hh_mc_solve_path(hhlib, name, anti):
    """every existing kind, both signs, all four barrier types: results, per-member payoffs and statistics =="""
    dyn, split, params = MODELS[name]
    m = _ffi.make_model(**params)
    for n, steps, every, start in SHAPES:
        c = config(dyn, n, steps, anti, split)
        payoffs, _, _ = base.every_kind(base.path_stats(hhlib, m, c, every, start))
        res, v, st = base.solve_path(hhlib, m, c, every, start, payoffs)
        res_x, v_x, st_x = solve_path_ex(hhlib, m, c, every, start, MONITORED, payoffs)
        assert [key(r) for r in res_x] == [key(r) for r in res], (name, anti, n)
        np.testing.assert_array_equal(v_x, v)
        np.testing.assert_array_equal(st_x, st)
        # … and under the bridge the kinds that read no extremes are what they were
        res_b, v_b, st_b = solve_path_ex(hhlib, m, c, every, start, BRIDGE, payoffs)
        np.testing.assert_array_equal(st_b[:5], st)
        for k, q in enumerate(payoffs):
            if q.kind != pc.BARRIER:
                assert key(res_b[k]) == key(res[k]), (name, anti, n, k)
                np.testing.assert_array_equal(v_b[k], v[k])


# ---- (2) the extremes against the 50-digit restatement, on live increments -------------------------------------------

@pytest.fixture(scope="module")
def oracle():
    return oracle_ffi.load()


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for k, (ratio, where) in sorted(w.items()):
        print(f"\npath_bridge (device) worst error/bar, {k}: {ratio:.3g} ({where})")


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(bc.LIVE))
def test_extremes_on_live_increments(hhlib, oracle, worst, name, anti):
    """The increments of 32 seeds filled on the device (hh_wiener_fill) and copied out, the bridge uniforms from the
    oracle's host Philox; the scheme and the header's bridge formulas on them at 50 digits.  S_T, CMAX_S and CMIN_S of
    every member within 20·max(e64, ε·A) (tests/path_bridge_cases.py).  Antithetic: the mirror's CMAX_S is ALSO compared
    with the reference that does not swap the two uniforms, which it must miss on most paths."""
    model, dyn, split, steps, _ = bc.LIVE[name]
    heston = dyn == "heston"
    dyn_c, ncomp = (HEST, 2) if heston else (LOGN, 1)
    n, seeds = bc.N_LIVE, bc.live_seeds(name)
    buf = _ffi.DeviceBuffer(hhlib, 8 * hhlib.lib.hh_replay_elems(n, steps, dyn_c))
    try:
        hhlib.check(hhlib.lib.hh_wiener_fill(hhlib.handle, dyn_c, model["rho"], model["T"], steps, n, seeds.ctypes.data, 0, buf.ptr))
        hhlib.synchronize()
        tiled = buf.download(np.empty(buf.nbytes // 8))
    finally:
        buf.free()
    case = bc.live_case(name, anti, bc.increments_of(tiled, n, steps, ncomp))
    ref = bc.reference(case, bc.bridge_uniforms(oracle, seeds, steps))
    left_out = n - int(ref["usable"].sum())
    print(f"\n{name} antithetic={anti}: {left_out} of {n} paths left out, clip fraction {ref['clip_fraction']:.3f}")
    assert left_out <= bc.MAX_UNUSABLE * n
    if name == "heston-classic-clipped":
        assert ref["clip_fraction"] >= bc.MIN_CLIP_FRACTION
    m = _ffi.make_model(S0=model["S0"], V0=model["V0"], kappa=model["kappa"], theta=model["theta"], sigma=model["sigma"],
                        rho=model["rho"], r=model["r_drift"], T=model["T"])
    c = _ffi.make_config(dyn_c, EULER, n, steps, antithetic=anti, em_split=split, seeds=seeds)
    stats = path_stats_ex(hhlib, m, c, 1, 1, BRIDGE)
    bars = bc.bar(ref["e64"], ref["A"])
    bad, unswapped_misses = [], 0
    for mem in range(ref["members"]):
        for i in np.flatnonzero(ref["usable"]):
            for slot, row in enumerate((pc.S_T, bc.CMAX_S, bc.CMIN_S)):
                got, want, b = stats[row, mem * n + i], ref["want"][mem][i][slot], bars[mem, i, slot]
                e = float(abs(bc.mp.mpf(float(got)) - want))
                kind = ("S_T", "CMAX_S", "CMIN_S")[slot]
                if e / b > worst.get(kind, (-1.0, ""))[0]:
                    worst[kind] = (e / b, f"{name} anti={anti} member {mem} path {i}")
                if not e <= b:
                    bad.append(f"{kind} member {mem} path {i}: got {got!r} want {bc.mp.nstr(want, 20)} error/bar {e / b:.3g}")
            if mem == 1:
                e = float(abs(bc.mp.mpf(float(stats[bc.CMAX_S, n + i])) - ref["wrong_cmax"][i]))
                unswapped_misses += int(e > bars[1, i, 1])
    assert not bad, "\n".join(bad[:20])
    if anti:
        print(f"{name}: the mirror's CMAX_S misses the unswapped reference on {unswapped_misses} of {n} paths")
        assert unswapped_misses > n / 2


# ---- (3) order -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(MODELS))
def test_continuous_extremes_bound_the_discrete_ones(hhlib, name, anti):
    """every = 1 with the start: the dates are all the states the continuous extremes range over, and cmax >= every state
    exactly; the slack is two exp roundings"""
    dyn, split, params = MODELS[name]
    m = _ffi.make_model(**params)
    for n, steps, _, _ in SHAPES:
        st = path_stats_ex(hhlib, m, config(dyn, n, steps, anti, split), 1, 1, BRIDGE)
        assert np.all(st[bc.CMAX_S] >= st[pc.MAX_S] * (1 - 2 * U)), (name, anti, n, steps)
        assert np.all(st[bc.CMIN_S] <= st[pc.MIN_S] * (1 + 2 * U)), (name, anti, n, steps)
        if steps > 1 and n > 100 and name != "heston-classic-clipped":  # … and strictly on nearly every path
            assert (st[bc.CMAX_S] > st[pc.MAX_S]).mean() > 0.9 and (st[bc.CMIN_S] < st[pc.MIN_S]).mean() > 0.9


# ---- (4) closed forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lognormal", "heston-split-sigma0", "heston-classic-sigma0"])
def test_closed_forms_of_continuous_monitoring(hhlib, name):
    """Up-and-out call (Reiner–Rubinstein), up-and-in through in/out parity, floating lookback call (Goldman–Sosin–
    Gatto): S0 = K = 100, B = 120, r = 0.05, vol 0.2, T = 1 on 16 steps, 2^18 trajectories.  Under lognormal dynamics
    the bridge is exact in law: |z| <= 4.  On the discrete extremes of the same seeds: |z| >= 10.  The Heston kernels
    with sigma = 0, V0 = theta = 0.04 have a constant variance: the same law through the other code path."""
    S0, K, B, r, vol, T, steps, n = 100.0, 100.0, 120.0, 0.05, 0.2, 1.0, 16, 2**18
    if name == "lognormal":
        dyn, split, m = LOGN, 1, _ffi.make_model(S0=S0, sigma=vol, r=r, T=T)
    else:
        dyn, split = HEST, int(name == "heston-split-sigma0")
        m = _ffi.make_model(S0=S0, V0=vol * vol, kappa=2.0, theta=vol * vol, sigma=0.0, rho=-0.7, r=r, T=T)
    c = config(dyn, n, steps, 0, split)
    payoffs = [pc.payoff(pc.BARRIER, K, 1.0, pc.UP_OUT, B), pc.payoff(pc.BARRIER, K, 1.0, pc.UP_IN, B),
               pc.payoff(bc.LB_FLOAT, 0.0, 1.0), pc.payoff(pc.VANILLA, K, 1.0)]
    out = bc.up_and_out_call(S0, K, B, r, vol, T)
    exact = [out, bc.bs_call(S0, K, r, vol, T) - out, bc.floating_lookback_call(S0, r, vol, T), bc.bs_call(S0, K, r, vol, T)]
    zs = {}
    for mode in (BRIDGE, MONITORED):
        arr, res = (_ffi.hh_path_payoff * 4)(*payoffs), (_ffi.hh_result * 4)()
        hhlib.check(hhlib.lib.hh_mc_solve_path_ex(hhlib.handle, C.byref(m), C.byref(c), 1, 1, mode, arr, 4, res, None, None))
        zs[mode] = [(res[k].price - exact[k]) / res[k].std_error for k in range(4)]
        for k in range(4):
            print(f"\n{name} extremes={mode} payoff {k}: price {res[k].price:.6f} exact {exact[k]:.6f} z {zs[mode][k]:+.2f}")
    for k in range(4):
        assert abs(zs[BRIDGE][k]) <= 4.0, (name, k, zs[BRIDGE][k])
    for k in range(3):
        assert abs(zs[MONITORED][k]) >= 10.0, (name, k, zs[MONITORED][k])
    assert abs(zs[MONITORED][3]) <= 4.0  # the vanilla reads no extremes


# ---- (5) identities and independence ---------------------------------------------------------------------------------

def sixteen(B, K=98.0, rebate=0.75):
    out = [pc.payoff(pc.VANILLA, K, cp) for cp in (1.0, -1.0)]
    out += [pc.payoff(pc.BARRIER, K, cp, t, B if t in (pc.UP_OUT, pc.UP_IN) else 0.85 * B, rebate)
            for t in (pc.UP_OUT, pc.UP_IN, pc.DOWN_OUT, pc.DOWN_IN) for cp in (1.0, -1.0)]
    out += [pc.payoff(bc.LB_FLOAT, 0.0, cp) for cp in (1.0, -1.0)]
    out += [pc.payoff(bc.LB_FIXED, K, cp) for cp in (1.0, -1.0)]
    out += [pc.payoff(pc.ARITH, K, 1.0), pc.payoff(pc.DCASH, K, -1.0, cash=2.0)]
    assert len(out) == 16
    return out


@pytest.mark.parametrize("mode", [BRIDGE, MONITORED])
@pytest.mark.parametrize("name", list(MODELS))
def test_identities_and_the_restatement_per_member(hhlib, name, mode):
    dyn, split, params = MODELS[name]
    n, steps, every, start, K, rebate = 513, 12, 3, 1, 98.0, 0.75
    m, c = _ffi.make_model(**params), config(dyn, n, steps, 1, split)
    row = bc.CMAX_S if mode == BRIDGE else pc.MAX_S
    B = float(np.median(path_stats_ex(hhlib, m, c, every, start, mode)[row]))
    payoffs = sixteen(B, K, rebate)
    res, v, st = solve_path_ex(hhlib, m, c, every, start, mode, payoffs)
    nm = pc.n_mon(steps, every, start)
    for k, q in enumerate(payoffs):  # the header's table on the returned statistics
        np.testing.assert_array_equal(v[k], bc.payoff_from_stats(st, q, nm, mode), err_msg=f"payoff {k} kind {q.kind}")
    for cp_i in (0, 1):
        van = v[cp_i]
        np.testing.assert_array_equal(v[2 + cp_i] + v[4 + cp_i], van + rebate)   # up: out + in
        np.testing.assert_array_equal(v[6 + cp_i] + v[8 + cp_i], van + rebate)   # down
    assert 0 < (v[2] == rebate).sum() < v[2].size
    assert np.all(v[10] >= 0.0) and np.all(v[11] >= 0.0)        # floating lookbacks
    assert np.all(v[12] >= v[0]) and np.all(v[13] >= v[1])      # fixed lookback >= vanilla, call and put
    assert (v[12] > v[0]).any()


def test_a_payoff_does_not_depend_on_what_else_is_in_the_call(hhlib):
    """16 payoffs (four workgroup groups) in one call and each alone, two chunks of the payoff kernel (n > 4096), both
    modes: results and per-member payoffs bit-identical"""
    n, steps, every, start = 4096 + 513, 6, 2, 1
    m, c = _ffi.make_model(), config(HEST, n, steps, 1)
    for mode in (BRIDGE, MONITORED):
        row = bc.CMAX_S if mode == BRIDGE else pc.MAX_S
        payoffs = sixteen(float(np.median(path_stats_ex(hhlib, m, c, every, start, mode)[row])))
        res16, v16, _ = solve_path_ex(hhlib, m, c, every, start, mode, payoffs)
        assert len({key(r) for r in res16}) == 16
        for lo, hi in [(k, k + 1) for k in range(16)] + [(5, 14), (11, 13)]:
            res, v, _ = solve_path_ex(hhlib, m, c, every, start, mode, payoffs[lo:hi])
            for j, k in enumerate(range(lo, hi)):
                assert key(res[j]) == key(res16[k]), (mode, lo, hi, k)
                np.testing.assert_array_equal(v[j], v16[k])


# ---- (6) argument errors ---------------------------------------------------------------------------------------------

def error_rows():
    """tests/test_gpu_path_payoff.py's table under the new names; kinds 6 and 7 are admitted here, 8 and -1 are not"""
    rows = []
    for r in base.error_rows():
        if r["id"] == "kind":
            r = dict(r, payoffs=[pc.payoff(8)], text=r["text"].replace("unknown kind 6", "unknown kind 8"))
        who = "hh_mc_path_stats" if r["stats_only"] else "hh_mc_solve_path"
        assert who in r["text"]
        rows.append(dict(r, text=r["text"].replace(who, who + "_ex"), extremes=MONITORED if len(rows) % 2 else BRIDGE))
    base_row = dict(cfg={}, every=2, payoffs=None, n_payoffs=None, null=None)
    rows.append(dict(base_row, id="extremes", code=INV, text="hh_mc_solve_path_ex: unknown extremes 2", extremes=2, stats_only=False))
    rows.append(dict(base_row, id="extremes.negative", code=INV, text="hh_mc_solve_path_ex: unknown extremes -1", extremes=-1, stats_only=False))
    rows.append(dict(base_row, id="stats.extremes", code=INV, text="hh_mc_path_stats_ex: unknown extremes 7", extremes=7, stats_only=True))
    return rows


def test_argument_errors_leave_the_context_usable():
    ctx = _ffi.Context(0)
    try:
        n, steps = 10, 4
        seeds = seeds_for(n)
        host = np.zeros(_ffi.HH_PATH_STATS_BRIDGE * n)
        out = (_ffi.hh_result * 2)()
        good = (_ffi.hh_path_payoff * 1)(pc.payoff(bc.LB_FLOAT))
        m = _ffi.make_model()
        rows = error_rows()
        assert {"kind", "kind.negative", "extremes", "stats.extremes", "replay", "partials", "exact_law"} <= {r["id"] for r in rows}
        for row in rows:
            kw = dict(row["cfg"])
            c = _ffi.make_config(kw.pop("dyn", HEST), kw.pop("strat", EULER), n, steps, seeds=seeds, **kw)
            if c.noise_mode == _ffi.HH_NOISE_REPLAY:
                c.replay, c.replay_len = host.ctypes.data, host.size
            null = row["null"]
            pm, pcfg = (None if null == "model" else C.byref(m)), (None if null == "cfg" else C.byref(c))
            if row["stats_only"]:
                rc = ctx.lib.hh_mc_path_stats_ex(ctx.handle, pm, pcfg, row["every"], 0, row["extremes"],
                                                 None if null == "stats" else host.ctypes.data, 0, None)
            else:
                ps = row["payoffs"]
                arr = (_ffi.hh_path_payoff * len(ps))(*ps) if ps else good
                k = row["n_payoffs"] if row["n_payoffs"] is not None else len(arr)
                rc = ctx.lib.hh_mc_solve_path_ex(ctx.handle, pm, pcfg, row["every"], 0, row["extremes"],
                                                 None if null == "payoffs" else arr, k, None if null == "out" else out, None, None)
            assert rc == row["code"], (row["id"], rc)
            assert ctx.lib.hh_last_error(ctx.handle).decode() == row["text"], row["id"]
            # the context still solves
            c = _ffi.make_config(HEST, EULER, n, steps, seeds=seeds)
            ctx.check(ctx.lib.hh_mc_solve_path_ex(ctx.handle, C.byref(m), C.byref(c), 2, 0, BRIDGE, good, 1, out, None, None))
            assert out[0].price > 0.0 and out[0].n_paths_done == n
        # the old entry point still refuses the lookbacks
        rc = ctx.lib.hh_mc_solve_path(ctx.handle, C.byref(m), C.byref(c), 2, 0, good, 1, out, None, None)
        assert rc == INV and ctx.lib.hh_last_error(ctx.handle).decode() == "hh_mc_solve_path: payoff 0: unknown kind 6"
    finally:
        ctx.close()


# ---- (7) the Python layer --------------------------------------------------------------------------------------------

REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
CONT = hh.ContinuousMonitoring()


def python_payoffs():
    m3 = hh.Monitoring(3, True)
    return [(hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), rebate=1.0, monitoring=CONT), BRIDGE),
            (hh.BarrierOption(100.0, 90.0, EXP, hh.Put(), hh.DownAndIn(), monitoring=CONT), BRIDGE),
            (hh.LookbackOption(EXP, hh.Call(), monitoring=CONT), BRIDGE),
            (hh.LookbackOption(EXP, hh.Put(), 100.0, CONT), BRIDGE),
            (hh.LookbackOption(EXP, hh.Put(), monitoring=m3), MONITORED),
            (hh.LookbackOption(EXP, hh.Call(), 100.0, m3), MONITORED)]


@pytest.mark.parametrize("anti", [False, True])
def test_solve_on_each_new_payoff_is_the_cabi_result(hhlib, anti):
    from hedgehog_jl_amd.montecarlo import _path_structs, pack_path_payoff
    mkt = hh.HestonInputs(REF, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    n = 700
    cfg = hh.SimulationConfig(n, steps=12, seeds=seeds_for(n), variance_reduction=hh.Antithetic() if anti else hh.NoVarianceReduction())
    mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    for p, mode in python_payoffs():
        sol = hh.solve(hh.PricingProblem(p, mkt), mc)
        model, c, every, start, _ = _path_structs([p], mkt, mc)
        assert (every, start) == ((12, False) if mode == BRIDGE else (3, True))
        c.seeds, c.seeds_len = cfg.seeds.ctypes.data, cfg.seeds.size
        res, _, stats = solve_path_ex(hhlib, model, c, every, int(start), mode, [pack_path_payoff(p)])
        assert (sol.price, sol.std_error) == (res[0].price, res[0].std_error) and sol.price > 0.0
        assert sol.ensemble.shape == (7 if mode == BRIDGE else 5, 2 * n if anti else n)
        np.testing.assert_array_equal(sol.ensemble, stats)
        assert hh.solve(hh.PricingProblem(p, mkt), mc, ensemble=False).ensemble is None


def test_baskets_group_by_extremes_mode(hhlib):
    mkt = hh.HestonInputs(REF, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    n = 700
    cfg = hh.SimulationConfig(n, steps=12, seeds=seeds_for(n), variance_reduction=hh.Antithetic())
    mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    asian = hh.AsianOption(100.0, EXP, hh.Call(), hh.ArithmeticAverage(), hh.Monitoring(1))
    cont = hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=CONT)
    disc = hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=hh.Monitoring(1))
    digital = hh.DigitalOption(100.0, EXP, hh.Call(), hh.CashOrNothing(5.0))
    look = hh.LookbackOption(EXP, hh.Call(), monitoring=CONT)
    from hedgehog_jl_amd.basket import path_groups
    for payoffs, n_groups in (([asian, cont, digital], 1), ([disc, cont], 2), ([asian, disc, look, cont, digital], 2)):
        assert len(path_groups(payoffs, 12)) == n_groups
        basket = hh.solve(hh.BasketPricingProblem(payoffs, mkt), mc, ensemble=True)
        for p, sol in zip(payoffs, basket.solutions):
            single = hh.solve(hh.PricingProblem(p, mkt), mc, ensemble=False)
            assert sol.problem.payoff is p
            assert (sol.price, sol.std_error) == (single.price, single.std_error), p
        if n_groups == 1:  # one simulation: the three share one seven-row ensemble
            assert all(s.ensemble is basket.solutions[0].ensemble for s in basket.solutions)
            assert basket.solutions[0].ensemble.shape == (7, 2 * n)
    # a continuous barrier is knocked out on more paths than a discrete one on the same trajectories
    two = hh.solve(hh.BasketPricingProblem([disc, cont], mkt), mc).solutions
    assert two[1].price < two[0].price
