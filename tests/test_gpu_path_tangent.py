"""Pathwise derivatives of the path payoffs on the device (hh_mc_path_stats_tangent, hh_mc_solve_path_tangent;
path_tangent_kernel and path_payoff_tangent_kernel, csrc/hh_path.hip).

(1) rows 0-4 are hh_mc_path_stats'; (2) the date rows exact and every tangent row of every carried slot within its bar of
the 50-digit restatement (tests/path_tangent_cases.py), path by path, on live increments, for n_active = 0 .. 4; (3) the
solve: price sums == hh_mc_solve_path(_ex)'s, every direction within the sum and assembly bars, a payoff independent of
what else is in the call; (4) the vanilla kind against hh_mc_solve's ForwardAD partials; (5) one statistical row against
the closed form of the discrete geometric Asian, with a wrong-rule control; (6) the refusals and the Python route."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex
from tests import euler_tangent_cases as tc
from tests import path_bridge_cases as bc
from tests import path_payoff_cases as pc
from tests import path_tangent_cases as tg
from tests import test_gpu_path_payoff as base

pytestmark = pytest.mark.gpu

LOGN, HEST, EULER = base.LOGN, base.HEST, base.EULER
INV, UNS = base.INV, base.UNS
SLOTS, NS = tg.SLOTS, tg.NS
BASIS_NAME = {_ffi.HH_BASIS_V0: "V0", _ffi.HH_BASIS_KAPPA: "kappa", _ffi.HH_BASIS_THETA: "theta", _ffi.HH_BASIS_SIGMA: "sigma"}
# the carried parameters of a call, by its seeds: every P = 0 .. 4 of the tangent kernel (lognormal dynamics carry sigma alone)
CARRIED = {"heston": ((), ("sigma",), ("V0", "theta"), ("kappa", "theta", "sigma"), ("V0", "kappa", "theta", "sigma")),
           "lognormal": ((), ("sigma",))}


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def model(case, seeds=None, n_partials=0, strike=100.0, cp=1.0):
    return _ffi.make_model(S0=case["S0"], V0=case["V0"], kappa=case["kappa"], theta=case["theta"], sigma=case["sigma"],
                           rho=case["rho"], r=case["r_drift"], T=case["T"], strike=strike, cp=cp, discount=case["discount"],
                           seeds=seeds, n_partials=n_partials)


def config(case, seeds, n_partials=0):
    return _ffi.make_config(tc.dyn_of(case), EULER, len(seeds), case["n_steps"], antithetic=int(case["antithetic"]),
                            em_split=int(case["em_split"]), seeds=seeds, n_partials=n_partials)


def unit_seeds(names):
    """direction k = a unit seed on names[k]; a call with no name seeds S0 alone (n_active = 0)"""
    names = names or ("S0",)
    return {n: [1.0 if j == k else 0.0 for j in range(len(names))] for k, n in enumerate(names)}, len(names)


def tangent_rows(ctx, m, c, every, start):
    """-> (rows (8 + 5·n_active, n_total), the carried parameters' names)"""
    rows = np.full((int(ctx.lib.hh_path_tangent_rows(_ffi.HH_TANGENT_MAX_BASIS)), n_total(c)), np.nan)
    basis, res = (C.c_int32 * 4)(), _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_tangent(ctx.handle, C.byref(m), C.byref(c), every, start, rows.ctypes.data, 0, basis,
                                               C.byref(res)))
    assert res.n_paths_done == c.n_paths and res.kernel_ms > 0.0
    names = [BASIS_NAME[b] for b in basis if b >= 0]
    n_rows = int(ctx.lib.hh_path_tangent_rows(len(names)))
    flat = rows.reshape(-1)[:n_rows * n_total(c)].reshape(n_rows, n_total(c))
    assert np.all(np.isnan(rows.reshape(-1)[n_rows * n_total(c):]))  # nothing written beyond the call's rows
    return flat, names


def solve_tangent(ctx, m, c, every, start, payoffs, n_active=None):
    K = len(payoffs)
    arr, res = (_ffi.hh_path_payoff * K)(*payoffs), (_ffi.hh_result * K)()
    rows = None if n_active is None else np.empty((int(ctx.lib.hh_path_tangent_rows(n_active)), n_total(c)))
    ctx.check(ctx.lib.hh_mc_solve_path_tangent(ctx.handle, C.byref(m), C.byref(c), every, start, arr, K, res,
                                               None if rows is None else rows.ctypes.data))
    return list(res), rows


def solve_plain(ctx, m, c, every, start, payoffs):
    K = len(payoffs)
    arr, res = (_ffi.hh_path_payoff * K)(*payoffs), (_ffi.hh_result * K)()
    ctx.check(ctx.lib.hh_mc_solve_path_ex(ctx.handle, C.byref(m), C.byref(c), every, start, _ffi.HH_EXTREMES_MONITORED, arr, K,
                                          res, None, None))
    return list(res)


def sums(r):
    return (r.price, r.std_error, r.sum_payoff, r.sumsq_payoff, r.n_paths_done)


def packed(case):
    return [pc.payoff(kind, K, cp) for kind, (K, cp) in zip(case["kinds"], case["payoff_list"])]


_dW = {}


def device_increments(ctx, name, steps):
    """the increments of the model's seeds filled on the device (hh_wiener_fill) and copied out, once per process"""
    if (name, steps) not in _dW:
        m, dyn, _, _ = tg.MODELS[name]
        dyn_c, ncomp = (HEST, 2) if dyn == "heston" else (LOGN, 1)
        seeds = tg.seeds_of(name)
        buf = _ffi.DeviceBuffer(ctx, 8 * ctx.lib.hh_replay_elems(tg.N_PATHS, steps, dyn_c))
        try:
            ctx.check(ctx.lib.hh_wiener_fill(ctx.handle, dyn_c, m["rho"], m["T"], steps, tg.N_PATHS, seeds.ctypes.data, 0, buf.ptr))
            ctx.synchronize()
            tiled = buf.download(np.empty(buf.nbytes // 8))
        finally:
            buf.free()
        _dW[(name, steps)] = bc.increments_of(tiled, tg.N_PATHS, steps, ncomp)
    return _dW[(name, steps)]


def cases_of(ctx, name, anti):
    for shape in tg.SHAPES:
        dW = device_increments(ctx, name, shape[0])
        for start in (0, 1):
            yield tg.case_of(name, shape, start, anti, dW)


@pytest.fixture(scope="module")
def worst():
    w = tc.Worst("path_tangent (device)")
    yield w
    w.report()


# ---- (1), (2) the rows -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(tg.MODELS))
def test_rows_against_the_restatement(hhlib, worst, name, anti):
    """Every case, every set of carried slots: rows 0-4 == hh_mc_path_stats; K_MAX, K_MIN == the reference's dates on the
    paths whose comparisons are decided; SUM_KS and the five tangent rows of every carried slot within
    20·max(e64, ε·A), member by member; the slots come out in the order V0, kappa, theta, sigma."""
    seeds = tg.seeds_of(name)
    n = tg.N_PATHS
    for case in cases_of(hhlib, name, anti):
        ref = tg.reference(case)
        every, start = case["monitor_every"], case["include_start"]
        assert n - int(ref["usable_sim"].sum()) <= tg.MAX_UNUSABLE * n
        five = base.path_stats(hhlib, model(case), config(case, seeds), every, start)
        bad = []
        for carried in CARRIED[case["dynamics"]]:
            sd, P = unit_seeds(carried)
            rows, names = tangent_rows(hhlib, model(case, sd, P), config(case, seeds, P), every, start)
            assert tuple(names) == carried and rows.shape == (8 + 5 * len(carried), five.shape[1])
            np.testing.assert_array_equal(rows[:5], five, err_msg=case["id"])
            for mem in range(ref["members"]):
                for i in np.flatnonzero(ref["usable_sim"]):
                    col = mem * n + i
                    where = f"{case['id']} carried={carried} member {mem} path {i}"
                    assert rows[_ffi.HH_TANGENT_K_MAX, col] == ref["k_max"][mem][i], where
                    assert rows[_ffi.HH_TANGENT_K_MIN, col] == ref["k_min"][mem][i], where
                    st = ref["stat"]["SUM_KS"]
                    bad.append(worst.check("SUM_KS", rows[_ffi.HH_TANGENT_SUM_KS, col], st["want"][mem][i][0],
                                           tc.path_bar(st["e64"][mem, i, 0], st["A"][mem, i, 0]), where))
                    for b, pname in enumerate(names):
                        s = 1 + SLOTS.index(pname)
                        for t, stat in enumerate(tg.STATS):
                            st = ref["stat"][stat]
                            bad.append(worst.check(f"d{stat}", rows[8 + 5 * b + t, col], st["want"][mem][i][s],
                                                   tc.path_bar(st["e64"][mem, i, s], st["A"][mem, i, s]), f"{where} d/d{pname}"))
        bad = [b for b in bad if b]
        assert not bad, "\n".join(bad[:20])


# ---- (3) the solve -----------------------------------------------------------------------------------------------------

MIXED = ([0.5, -2.0, 0.25, 1.5, -0.75, 3.0, -0.5, 0.125], [-1.0, 0.0, 0.0, 4.0, 0.0, -0.25, 1.0, -2.0])


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(tg.MODELS))
def test_solve_against_the_restatement(hhlib, worst, name, anti):
    """On the seeds of the paths every payoff's comparisons are decided on: price, std_error and both sums ==
    hh_mc_solve_path_ex's (monitored extremes: hh_mc_solve_path for its kinds); the eight unit directions within the sum
    bars (euler_tangent_cases.check_solve, as hh_mc_solve's partials are held); two mixed directions, seeds on all eight
    slots — ddiscount and dstrike among them — within Σ|seed|·bar."""
    all_seeds = tg.seeds_of(name)
    for case in cases_of(hhlib, name, anti):
        ref = tg.reference(case)
        paths = [int(i) for i in np.flatnonzero(ref["usable_all"])]
        n = len(paths)
        assert tg.N_PATHS - n <= tg.MAX_UNUSABLE * tg.N_PATHS
        seeds = all_seeds[paths]
        every, start, payoffs = case["monitor_every"], case["include_start"], packed(case)
        plain = solve_plain(hhlib, model(case), config(case, seeds), every, start, payoffs)
        res, _ = solve_tangent(hhlib, model(case, tc.UNIT, NS), config(case, seeds, NS), every, start, payoffs)
        mixed_seeds = {s: [MIXED[0][k], MIXED[1][k]] for k, s in enumerate(SLOTS)}
        mix, _ = solve_tangent(hhlib, model(case, mixed_seeds, 2), config(case, seeds, 2), every, start, payoffs)
        bad = []
        for j, pj in enumerate(ref["payoffs"]):
            assert sums(res[j]) == sums(plain[j]) == sums(mix[j]), (case["id"], j)
            if tg.n_mon_of(case) == 1 and case["kinds"][j] == tg.LB_FLOAT:  # S_T − S_T: exact zeros
                assert res[j].price == 0.0 and not any(res[j].dprice) and not any(mix[j].dprice), case["id"]
                continue
            bad += tc.check_solve(worst, case, ref, j, paths, res[j], None, f"kind {case['kinds'][j]}")
            price, bar = tc.sum_of(pj["price"], pj["price_e64"], pj["price_A"], paths, anti)
            for k in range(2):
                want, b = tc.assembled(MIXED[k], price, bar)
                with mp.workdps(ex.DPS):
                    want = want / n
                bad.append(worst.check("mixed direction", mix[j].dprice[k], want, b / n, f"{case['id']} payoff {j} direction {k}"))
            assert not any(mix[j].dprice[2:])
        bad = [b for b in bad if b]
        assert not bad, "\n".join(bad[:20])


def test_a_payoff_does_not_depend_on_what_else_is_in_the_call(hhlib):
    """16 payoffs (four workgroup groups) in one call and in 16 calls of one: every result bit for bit, dprice included;
    two chunks of the payoff kernel, antithetic, four carried slots."""
    n, steps, every, start = 4099, 12, 3, 1
    case = dict(tg.H, dynamics="heston", em_split=1, n_steps=steps, antithetic=1)
    seeds = base.seeds_for(n)
    payoffs = [pc.payoff(kind, K, cp) for kind in (pc.VANILLA, pc.ARITH, pc.GEOM, tg.LB_FIXED) for K, cp in
               ((95.0, 1.0), (105.0, 1.0), (100.0, -1.0))] + [pc.payoff(tg.LB_FLOAT, 0.0, 1.0), pc.payoff(tg.LB_FLOAT, 0.0, -1.0),
                                                               pc.payoff(pc.ARITH, 100.0, 1.0), pc.payoff(pc.GEOM, 101.0, -1.0)]
    assert len(payoffs) == 16
    m, c = model(case, tc.UNIT, NS), config(case, seeds, NS)
    together, _ = solve_tangent(hhlib, m, c, every, start, payoffs)
    for k, q in enumerate(payoffs):
        alone, _ = solve_tangent(hhlib, m, c, every, start, [q])
        assert sums(alone[0]) + tuple(alone[0].dprice) == sums(together[k]) + tuple(together[k].dprice), k
        assert any(together[k].dprice)


# ---- (4) the vanilla kind is hh_mc_solve's ForwardAD pass ---------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(tg.MODELS))
def test_vanilla_kind_against_forward_ad_of_the_terminal_solve(hhlib, name, anti):
    """The same trajectories (the same seeds, GENERATE noise), the same eight unit seeds: every partial of the vanilla kind
    within the reference's sum bar of hh_mc_solve's, and the price sums ==."""
    all_seeds = tg.seeds_of(name)
    for case in cases_of(hhlib, name, anti):
        ref = tg.reference(case)
        paths = [int(i) for i in np.flatnonzero(ref["usable_all"])]
        seeds, n = all_seeds[paths], len(paths)
        for j, kind in enumerate(case["kinds"]):
            if kind != tg.VANILLA:
                continue
            K, cp = case["payoff_list"][j]
            res, _ = solve_tangent(hhlib, model(case, tc.UNIT, NS), config(case, seeds, NS), case["monitor_every"],
                                   case["include_start"], [pc.payoff(kind, K, cp)])
            ad = _ffi.hh_result()
            m, c = model(case, tc.UNIT, NS, strike=K, cp=cp), config(case, seeds, NS)
            hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(ad), None))
            assert (res[0].price, res[0].sum_payoff, res[0].sumsq_payoff) == (ad.price, ad.sum_payoff, ad.sumsq_payoff)
            pj = ref["payoffs"][j]
            _, bar = tc.sum_of(pj["price"], pj["price_e64"], pj["price_A"], paths, anti)
            for k in range(NS):
                assert abs(res[0].dprice[k] - ad.dprice[k]) <= bar[1 + k] / n, (case["id"], j, SLOTS[k])


# ---- (5) one statistical row -------------------------------------------------------------------------------------------

def geometric_asian_call(S0, sigma, K, r, T, steps, every, start):
    """The discretely monitored geometric Asian call under lognormal dynamics: ln G = mean of ln S on the dates is
    normal — mean ln S0 + (r − σ²/2)·mean(t_j), variance σ²·ΣΣ min(t_i, t_j)/n² — so the price is Black's formula on it."""
    dt = mp.mpf(T) / steps
    ts = ([mp.mpf(0)] if start else []) + [dt * every * j for j in range(1, steps // every + 1)]
    n = len(ts)
    mu = mp.log(S0) + (r - sigma * sigma / 2) * mp.fsum(ts) / n
    var = sigma * sigma * mp.fsum(min(a, b) for a in ts for b in ts) / (n * n)
    sd = mp.sqrt(var)
    d2 = (mu - mp.log(K)) / sd
    return mp.exp(-mp.mpf(r) * T) * (mp.exp(mu + var / 2) * mp.ncdf(d2 + sd) - K * mp.ncdf(d2))


def test_geometric_asian_delta_and_vega_against_the_closed_form(hhlib):
    """Lognormal, 16 steps (the Euler step on the log state is the exact transition), 2¹⁶ trajectories: delta and vega
    within 4 standard errors of the closed form's derivatives (mpmath.diff), the standard error formed in numpy from the
    returned rows.  Control: the terminal tangent in place of the average's — the vanilla's rule on the Asian's itm set —
    misses by more than 4 standard errors."""
    S0, sigma, K, r, T, steps, n = 100.0, 0.2, 100.0, 0.05, 1.0, 16, 2**16
    case = dict(S0=S0, V0=0.0, kappa=0.0, theta=0.0, sigma=sigma, rho=0.0, r_drift=r, T=T, discount=float(np.exp(-r * T)),
                dynamics="lognormal", em_split=1, n_steps=steps, antithetic=0)
    seeds = base.seeds_for(n)
    sd = dict(S0=[1.0, 0.0], sigma=[0.0, 1.0])
    res, rows = solve_tangent(hhlib, model(case, sd, 2), config(case, seeds, 2), 1, 0, [pc.payoff(pc.GEOM, K, 1.0)], n_active=1)
    with mp.workdps(30):
        delta = float(mp.diff(lambda s: geometric_asian_call(s, mp.mpf(sigma), K, r, T, steps, 1, 0), S0))
        vega = float(mp.diff(lambda v: geometric_asian_call(mp.mpf(S0), v, K, r, T, steps, 1, 0), sigma))
    D, n_mon = case["discount"], float(steps)
    G = np.exp(rows[pc.SUM_X] / n_mon)
    itm = (G - K > 0.0).astype(float)
    dsum_x = {"delta": np.full(n, n_mon / S0), "vega": rows[8 + _ffi.HH_TANGENT_DSUM_X]}
    ds_t = {"delta": rows[pc.S_T] / S0, "vega": rows[8 + _ffi.HH_TANGENT_DS_T]}
    for k, (greek, exact) in enumerate((("delta", delta), ("vega", vega))):
        sample = D * itm * G * dsum_x[greek] / n_mon
        se = sample.std(ddof=1) / np.sqrt(n)
        assert res[0].dprice[k] == pytest.approx(sample.mean(), rel=1e-12)
        z = (res[0].dprice[k] - exact) / se
        wrong = (D * itm * ds_t[greek]).mean()
        z_wrong = (wrong - exact) / se
        print(f"\ngeometric Asian {greek}: {res[0].dprice[k]:.6f}, closed form {exact:.6f}, z = {z:+.2f}; terminal tangent: z = {z_wrong:+.2f}")
        assert abs(z) <= 4.0, greek
        assert abs(z_wrong) > 4.0, greek


# ---- (6) refusals, and the Python route --------------------------------------------------------------------------------

def error_rows():
    who = "hh_mc_solve_path_tangent"
    jump = f"{who}: payoff 0 (kind %d) is discontinuous: its pathwise derivative omits the jump term — use FiniteDifference"
    one = lambda kind, **kw: [pc.payoff(kind, **kw)]  # noqa: E731
    return [
        ("barrier", UNS, jump % pc.BARRIER, dict(payoffs=one(pc.BARRIER, barrier_type=pc.UP_OUT, barrier=120.0))),
        ("digital-cash", UNS, jump % pc.DCASH, dict(payoffs=one(pc.DCASH, cash=1.0))),
        ("digital-asset", UNS, jump % pc.DASSET, dict(payoffs=one(pc.DASSET))),
        ("replay", UNS, f"{who}: GENERATE noise: the pathwise tangent has no REPLAY form", dict(cfg=dict(noise_mode=_ffi.HH_NOISE_REPLAY))),
        ("exact-law", UNS, f"{who} needs LognormalDynamics or HestonDynamics + EulerMaruyama",
         dict(cfg=dict(dyn=LOGN, strat=_ffi.HH_EXACT_LAW))),
        ("broadie-kaya", UNS, f"{who} needs LognormalDynamics or HestonDynamics + EulerMaruyama",
         dict(cfg=dict(strat=_ffi.HH_BROADIE_KAYA))),
        ("qe", UNS, f"{who} needs LognormalDynamics or HestonDynamics + EulerMaruyama", dict(cfg=dict(strat=_ffi.HH_QE))),
        ("no-partials", INV, f"{who}: n_partials (0) must be 1 .. 8", dict(cfg=dict(n_partials=0))),
        ("too-many-partials", INV, f"{who}: n_partials (9) must be 1 .. 8", dict(cfg=dict(n_partials=9))),
        ("null-model", INV, f"{who}: NULL argument", dict(null="model")),
        ("null-cfg", INV, f"{who}: NULL argument", dict(null="cfg")),
        ("null-payoffs", INV, f"{who}: NULL argument", dict(null="payoffs")),
        ("null-out", INV, f"{who}: NULL argument", dict(null="out")),
        ("every", INV, f"{who}: monitor_every (3) must be >= 1 and divide n_steps (4)", dict(every=3)),
        ("no-payoffs", INV, f"{who}: 1 .. 1024 payoffs", dict(n_payoffs=0)),
        ("kind", INV, f"{who}: payoff 0: unknown kind 8", dict(payoffs=one(8))),
        ("cp", INV, f"{who}: payoff 0: cp must be +1 or -1", dict(payoffs=one(pc.ARITH, cp=0.5))),
    ]


def test_refusals_leave_the_context_usable():
    ctx = _ffi.Context(0)
    try:
        n, steps = 10, 4
        seeds = base.seeds_for(n)
        host = np.zeros(8 * n * steps)
        out = (_ffi.hh_result * 1)()
        good = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.ARITH))
        sd = dict(sigma=[1.0])
        for rid, code, text, row in error_rows():
            kw = dict(dict(n_partials=1), **row.get("cfg", {}))
            c = _ffi.make_config(kw.pop("dyn", HEST), kw.pop("strat", EULER), n, steps, seeds=seeds, **kw)
            if c.noise_mode == _ffi.HH_NOISE_REPLAY:
                c.replay, c.replay_len = host.ctypes.data, host.size
            m = _ffi.make_model(seeds=sd, n_partials=1)
            null = row.get("null")
            ps = row.get("payoffs")
            arr = (_ffi.hh_path_payoff * len(ps))(*ps) if ps else good
            rc = ctx.lib.hh_mc_solve_path_tangent(ctx.handle, None if null == "model" else C.byref(m),
                                                  None if null == "cfg" else C.byref(c), row.get("every", 2), 0,
                                                  None if null == "payoffs" else arr, row.get("n_payoffs", len(arr)),
                                                  None if null == "out" else out, None)
            assert rc == code, (rid, rc)
            assert ctx.lib.hh_last_error(ctx.handle).decode() == text, rid
            c = _ffi.make_config(HEST, EULER, n, steps, seeds=seeds, n_partials=1)
            ctx.check(ctx.lib.hh_mc_solve_path_tangent(ctx.handle, C.byref(m), C.byref(c), 2, 0, good, 1, out, None))
            assert out[0].price > 0.0 and out[0].n_paths_done == n and out[0].dprice[0] != 0.0
        # the statistics entry point: its own name in the words, NULL rows
        c = _ffi.make_config(HEST, EULER, n, steps, seeds=seeds, n_partials=0)
        assert ctx.lib.hh_mc_path_stats_tangent(ctx.handle, C.byref(m), C.byref(c), 2, 0, host.ctypes.data, 0, None, None) == INV
        assert ctx.lib.hh_last_error(ctx.handle).decode() == "hh_mc_path_stats_tangent: n_partials (0) must be 1 .. 8"
        assert ctx.lib.hh_mc_path_stats_tangent(ctx.handle, C.byref(m), C.byref(c), 2, 0, None, 0, None, None) == INV
        assert ctx.lib.hh_last_error(ctx.handle).decode() == "hh_mc_path_stats_tangent: NULL argument"
        # … and the plain entry points still refuse partials in their words
        c = _ffi.make_config(HEST, EULER, n, steps, seeds=seeds, n_partials=1)
        assert ctx.lib.hh_mc_solve_path(ctx.handle, C.byref(m), C.byref(c), 2, 0, good, 1, out, None, None) == UNS
        assert ctx.lib.hh_last_error(ctx.handle).decode() == "hh_mc_solve_path: GENERATE noise, no dual partials"
    finally:
        ctx.close()


REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


@pytest.mark.parametrize("anti", [False, True])
def test_python_batch_of_five_heston_lenses_is_five_unit_seed_calls(hhlib, anti):
    n, steps = 700, 12
    mkt = hh.HestonInputs(REF, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    cfg = hh.SimulationConfig(n, steps=steps, seeds=base.seeds_for(n),
                              variance_reduction=hh.Antithetic() if anti else hh.NoVarianceReduction())
    mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    lenses = (hh.SpotLens(), hh.optic("market_inputs.V0"), hh.optic("market_inputs.κ"), hh.optic("market_inputs.θ"),
              hh.optic("market_inputs.σ"))
    names = ("S0", "V0", "kappa", "theta", "sigma")
    from hedgehog_jl_amd.montecarlo import _model_and_config, pack_path_payoff
    for payoff in (hh.AsianOption(100.0, EXP, hh.Call(), hh.ArithmeticAverage(), hh.Monitoring(3, True)),
                   hh.AsianOption(100.0, EXP, hh.Put(), hh.GeometricAverage(), hh.Monitoring(1, False)),
                   hh.LookbackOption(EXP, hh.Call(), None, hh.Monitoring(2, True)),
                   hh.LookbackOption(EXP, hh.Put(), 101.0, hh.Monitoring(3, False))):
        prob = hh.PricingProblem(payoff, mkt)
        batch = hh.solve(hh.BatchGreekProblem(prob, lenses), hh.Pathwise(), mc)
        assert list(batch) == list(lenses)
        european = hh.VanillaOption(1.0 if payoff.strike is None else payoff.strike, payoff.expiry, hh.European(), hh.Call(), hh.Spot())
        every, start = payoff.monitoring.every, int(payoff.monitoring.include_start)
        for lens, pname in zip(lenses, names):
            m, c, _, _, _ = _model_and_config(hh.PricingProblem(european, mkt), mc)
            seed = (C.c_double * 1)(1.0)
            setattr(m, "d" + pname, C.cast(seed, C.POINTER(C.c_double)))
            c.n_partials = 1
            c.seeds, c.seeds_len = cfg.seeds.ctypes.data, cfg.seeds.size
            res, _ = solve_tangent(hhlib, m, c, every, start, [pack_path_payoff(payoff)])
            assert batch[lens] == res[0].dprice[0] and batch[lens] != 0.0, (type(payoff).__name__, pname)
            single = hh.solve(hh.GreekProblem(prob, lens), hh.Pathwise(), mc)
            assert single.greek == res[0].dprice[0]
    # a European vanilla: ForwardAD's fused pass
    vanilla = hh.PricingProblem(hh.VanillaOption(100.0, EXP, hh.European(), hh.Call(), hh.Spot()), mkt)
    assert hh.solve(hh.BatchGreekProblem(vanilla, lenses), hh.Pathwise(), mc) == \
        hh.solve(hh.BatchGreekProblem(vanilla, lenses), hh.ForwardAD(), mc)
