"""Path-dependent payoffs on the device (hh_mc_path_stats, hh_mc_solve_path; csrc/hh_path.hip).

(a) the statistics against hh_euler_grid's rows, which are the same trajectories bit for bit; (b) every payoff kind
against the numpy restatement on those statistics, and every result against hh_mc_finalize on an accumulator built
from the per-member payoffs; (c) identities between payoffs, per path; (d) a payoff's result does not depend on what
else is in the call; (e) the closed forms that exist under lognormal dynamics; (f) the argument errors; (g) the Python
layer.  Shapes are the smallest at which the kernels can go wrong: a single trajectory, ragged last workgroups, odd
step counts (the tail of the lognormal two-steps-per-draw loop), more than one chunk of the payoff kernel."""
import ctypes as C
import math

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import path_payoff_cases as pc

pytestmark = pytest.mark.gpu

LOGN, HEST, EULER = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA
INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
FV = dict(V0=0.01, kappa=0.5, theta=0.02, sigma=1.0, rho=-0.9)  # 2κθ < σ²: the variance clips on many steps
MODELS = {"heston-split": (HEST, 1, {}), "heston-classic-clipped": (HEST, 0, FV), "lognormal": (LOGN, 1, dict(sigma=0.2))}
SHAPES = [(1, 1, 1, 0), (255, 7, 1, 1), (257, 7, 7, 0), (1000, 12, 3, 1), (513, 12, 4, 0)]
U = 2.0 ** -52


def seeds_for(n):
    return np.random.default_rng(20240607).integers(0, 2**64, size=n, dtype=np.uint64)


def config(dyn, n, steps, anti, split=1):
    return _ffi.make_config(dyn, EULER, n, steps, antithetic=anti, em_split=split, seeds=seeds_for(n))


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def euler_grid(ctx, m, c, state, want_var=False):
    spot = np.empty((c.n_steps + 1, n_total(c)))
    var = np.empty_like(spot) if want_var else None
    ctx.check(ctx.lib.hh_euler_grid(ctx.handle, C.byref(m), C.byref(c), state, spot.ctypes.data,
                                    var.ctypes.data if want_var else None, 0, None))
    return spot, var


def path_stats(ctx, m, c, every, start):
    stats = np.empty((_ffi.HH_PATH_STATS, n_total(c)))
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats(ctx.handle, C.byref(m), C.byref(c), every, start, stats.ctypes.data, 0, C.byref(res)))
    assert res.n_paths_done == c.n_paths and res.kernel_ms > 0.0
    return stats


def solve_path(ctx, m, c, every, start, payoffs):
    """-> (results, per-member payoffs (K, n_total), statistics (5, n_total))"""
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = np.empty((K, n_total(c))), np.empty((_ffi.HH_PATH_STATS, n_total(c)))
    ctx.check(ctx.lib.hh_mc_solve_path(ctx.handle, C.byref(m), C.byref(c), every, start, arr, K, res,
                                       values.ctypes.data, stats.ctypes.data))
    return list(res), values, stats


def samples_of(values_row, c):
    """the samples a payoff's sums run over: the members' payoffs, pair-averaged when antithetic (montecarlo.jl:431)"""
    n = int(c.n_paths)
    return (values_row[:n] + values_row[n:]) / 2 if c.antithetic else values_row


# ---- (a) the statistics against the grid ----------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("name", list(MODELS))
def test_statistics_are_those_of_the_grid_rows(hhlib, name, anti):
    dyn, split, params = MODELS[name]
    m = _ffi.make_model(**params)
    clipped = total = 0
    for n, steps, every, start in SHAPES:
        c = config(dyn, n, steps, anti, split)
        spot, var = euler_grid(hhlib, m, c, _ffi.HH_PATH_SPOT, want_var=dyn == HEST)
        logs, _ = euler_grid(hhlib, m, c, _ffi.HH_PATH_LOG)
        stats = path_stats(hhlib, m, c, every, start)
        rows = pc.monitored_rows(steps, every, start)
        assert len(rows) == pc.n_mon(steps, every, start)
        where = (name, anti, n, steps, every, start)
        np.testing.assert_array_equal(stats[pc.MAX_S], spot[rows].max(axis=0), err_msg=str(where))
        np.testing.assert_array_equal(stats[pc.MIN_S], spot[rows].min(axis=0), err_msg=str(where))
        np.testing.assert_array_equal(stats[pc.S_T], spot[steps], err_msg=str(where))
        sum_s, sum_x = spot[rows[0]].copy(), logs[rows[0]].copy()
        for r in rows[1:]:  # date order, one rounded addition per date
            sum_s = sum_s + spot[r]
            sum_x = sum_x + logs[r]
        np.testing.assert_array_equal(stats[pc.SUM_S], sum_s, err_msg=str(where))
        np.testing.assert_array_equal(stats[pc.SUM_X], sum_x, err_msg=str(where))
        # … and S_T is the terminal sample of the European solve on the same seeds
        term, res = np.empty(n_total(c)), _ffi.hh_result()
        hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(res), term.ctypes.data))
        np.testing.assert_array_equal(stats[pc.S_T], term, err_msg=str(where))
        if var is not None and steps >= 7:  # the variance states the steps read: rows 0 .. n_steps - 1
            clipped += int((var[:steps] <= 0.0).sum())
            total += var[:steps].size
    if name == "heston-classic-clipped":  # (a single step reads V0 > 0 alone: the shapes of 7 and 12 steps are counted)
        assert clipped >= 0.10 * total, (clipped, total)


# ---- (b) payoffs from the statistics ---------------------------------------------------------------------------------

def every_kind(stats):
    """every kind, both cp, all four barrier types with both cp; barrier levels from the statistics themselves, one of
    them exactly one trajectory's MAX_S (a touch)"""
    up = float(np.sort(stats[pc.MAX_S])[stats.shape[1] // 2])      # exactly one member's maximum
    down = float(np.quantile(stats[pc.MIN_S], 0.4))
    out = [pc.payoff(kind, 100.0, cp) for kind in (pc.VANILLA, pc.ARITH, pc.GEOM) for cp in (1.0, -1.0)]
    out += [pc.payoff(pc.BARRIER, 100.0, cp, t, up if t in (pc.UP_OUT, pc.UP_IN) else down, rebate=1.25)
            for t in (pc.UP_OUT, pc.UP_IN, pc.DOWN_OUT, pc.DOWN_IN) for cp in (1.0, -1.0)]
    out += [pc.payoff(pc.DCASH, 100.0, cp, cash=3.0) for cp in (1.0, -1.0)]
    out += [pc.payoff(pc.DASSET, 100.0, cp) for cp in (1.0, -1.0)]
    return out, up, down


@pytest.mark.parametrize("anti", [0, 1])
def test_every_payoff_kind_against_the_restatement_and_its_own_sums(hhlib, anti):
    """path_values == the numpy restatement on the returned statistics (the geometric average within the two
    exponentials' bounds: 1 ulp for the device library's exp, 1 ulp for numpy's, on avg = exp(SUM_X / n_mon)); each
    result against hh_mc_finalize on an accumulator summed in numpy from that payoff's samples.  Bounds: two fp64 sums
    of the same n terms in any two orders differ by at most (n - 1)·2^-52·Σ|p| (each is within (n - 1)·2^-53·Σ|p| of
    the exact sum); Σp² likewise with one more rounding per term for the product (n·2^-52·Σp²).  std_error =
    D·sqrt(var / n), var = (Σp² - (Σp)²/n)/(n - 1): the two bounds go through it to first order, d var <=
    (dΣp² + 2|Σp|·dΣp/n)/(n - 1), d se = D·d var/(2·sqrt(var·n)), plus 4 ulp for the formula's own roundings."""
    n, steps, every, start = 1000, 12, 3, 1
    m = _ffi.make_model()
    c = config(HEST, n, steps, anti)
    payoffs, up, down = every_kind(path_stats(hhlib, m, c, every, start))
    res, values, stats = solve_path(hhlib, m, c, every, start, payoffs)
    np.testing.assert_array_equal(stats, path_stats(hhlib, m, c, every, start))
    assert (stats[pc.MAX_S] == up).sum() >= 1
    for B, hit in ((up, stats[pc.MAX_S] >= up), (down, stats[pc.MIN_S] <= down)):
        assert 0.10 <= hit.mean() <= 0.90, (B, hit.mean())
    nm = pc.n_mon(steps, every, start)
    for k, q in enumerate(payoffs):
        want = pc.payoff_from_stats(stats, q, nm)
        if q.kind == pc.GEOM:
            bar = 2.0 * np.spacing(np.exp(stats[pc.SUM_X] / float(nm)))
            worst = float(np.max(np.abs(values[k] - want) / bar))
            print(f"\ngeometric average cp={q.cp:+.0f} antithetic={anti}: worst error/bar {worst:.3g}")
            assert worst <= 1.0
        else:
            np.testing.assert_array_equal(values[k], want, err_msg=f"payoff {k} kind {q.kind}")
        p = samples_of(values[k], c)
        acc = np.zeros(_ffi.HH_ACC_LEN)
        acc[_ffi.HH_ACC_SUM], acc[_ffi.HH_ACC_SUMSQ], acc[_ffi.HH_ACC_NPATHS] = np.sum(p), np.sum(p * p), n
        ref = _ffi.hh_result()
        assert hhlib.lib.hh_mc_finalize(C.byref(m), C.byref(c), acc.ctypes.data, C.byref(ref)) == 0
        d_sum, d_sq = (n - 1) * U * float(np.sum(np.abs(p))), n * U * float(np.sum(p * p))
        assert abs(res[k].sum_payoff - ref.sum_payoff) <= d_sum, k
        assert abs(res[k].sumsq_payoff - ref.sumsq_payoff) <= d_sq, k
        assert abs(res[k].price - ref.price) <= m.discount * d_sum / n + np.spacing(ref.price), k
        var = (ref.std_error / m.discount) ** 2 * n
        assert var > 0.0
        d_var = (d_sq + 2.0 * abs(ref.sum_payoff) * d_sum / n) / (n - 1)
        assert abs(res[k].std_error - ref.std_error) <= m.discount * d_var / (2.0 * math.sqrt(var * n)) + 4 * np.spacing(ref.std_error), k
        assert res[k].n_paths_done == n and not any(res[k].dprice) and res[k].kernel_ms > 0.0


# ---- (c) identities, per path ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["heston-split", "lognormal"])
def test_identities_between_payoffs(hhlib, name):
    dyn, split, params = MODELS[name]
    n, steps, every, start, anti, K, rebate = 513, 12, 3, 1, 1, 98.0, 0.75
    c = config(dyn, n, steps, anti, split)
    for cp in (1.0, -1.0):
        m = _ffi.make_model(strike=K, cp=cp, **params)
        B = float(np.median(path_stats(hhlib, m, c, every, start)[pc.MAX_S]))
        payoffs = [pc.payoff(pc.VANILLA, K, cp),
                   pc.payoff(pc.BARRIER, K, cp, pc.UP_OUT, B, rebate), pc.payoff(pc.BARRIER, K, cp, pc.UP_IN, B, rebate),
                   pc.payoff(pc.BARRIER, K, cp, pc.DOWN_OUT, 0.9 * B, rebate), pc.payoff(pc.BARRIER, K, cp, pc.DOWN_IN, 0.9 * B, rebate),
                   pc.payoff(pc.BARRIER, K, cp, pc.UP_OUT, math.inf, rebate), pc.payoff(pc.BARRIER, K, cp, pc.DOWN_OUT, 0.0, rebate)]
        res, v, stats = solve_path(hhlib, m, c, every, start, payoffs)
        van = v[0]
        np.testing.assert_array_equal(v[1] + v[2], van + rebate)   # knock-out + knock-in
        np.testing.assert_array_equal(v[3] + v[4], van + rebate)
        assert 0 < (v[1] == rebate).sum() < v[1].size
        np.testing.assert_array_equal(v[5], van)                   # a barrier that is never hit
        np.testing.assert_array_equal(v[6], van)
        # … and the vanilla is the European solve's payoff on its terminal samples, its price that solve's price
        term, eur = np.empty(n_total(c)), _ffi.hh_result()
        hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(eur), term.ctypes.data))
        mT = cp * (term - K)
        np.testing.assert_array_equal(van, np.where(mT > 0.0, mT, 0.0))
        d_sum = (n - 1) * U * float(np.sum(np.abs(samples_of(van, c))))
        for k in (0, 5, 6):
            assert abs(res[k].sum_payoff - eur.sum_payoff) <= d_sum
            assert abs(res[k].price - eur.price) <= m.discount * d_sum / n + np.spacing(eur.price)
        assert res[5].price == res[0].price == res[6].price and res[5].sumsq_payoff == res[0].sumsq_payoff
        # an average over the expiry date alone is the terminal sample
        res1, v1, st1 = solve_path(hhlib, m, c, steps, 0, [pc.payoff(pc.ARITH, K, cp), pc.payoff(pc.VANILLA, K, cp)])
        np.testing.assert_array_equal(v1[0], v1[1])
        np.testing.assert_array_equal(v1[1], van)
        np.testing.assert_array_equal(st1[pc.SUM_S], st1[pc.S_T])
        assert res1[0].price == res1[1].price == res[0].price
        # AM-GM (the geometric mean's own roundings: a division, an exp of 1 ulp, against n_mon additions and a division)
        nm = float(pc.n_mon(steps, every, start))
        assert np.all(stats[pc.SUM_S] / nm >= np.exp(stats[pc.SUM_X] / nm) * (1.0 - 4.0 * U))


# ---- (d) independence of grouping ------------------------------------------------------------------------------------

def test_a_payoff_does_not_depend_on_what_else_is_in_the_call(hhlib):
    """9 payoffs alone, in a call of 4, of 5 and of 9 (so that a payoff sits in different workgroup groups and at
    different places of a group): results and per-member payoffs bit-identical.  Two chunks of the payoff kernel."""
    n, steps, every, start = 4096 + 513, 6, 2, 1
    m, c = _ffi.make_model(), config(HEST, n, steps, 1)
    B = float(np.median(path_stats(hhlib, m, c, every, start)[pc.MAX_S]))
    payoffs = [pc.payoff(pc.ARITH, 100.0, 1.0), pc.payoff(pc.GEOM, 101.0, -1.0), pc.payoff(pc.BARRIER, 99.0, 1.0, pc.UP_OUT, B, 0.5),
               pc.payoff(pc.DCASH, 100.0, 1.0, cash=2.0), pc.payoff(pc.VANILLA, 102.0, -1.0), pc.payoff(pc.BARRIER, 100.0, -1.0, pc.DOWN_IN, 0.9 * B, 0.25),
               pc.payoff(pc.DASSET, 98.0, 1.0), pc.payoff(pc.GEOM, 97.0, 1.0), pc.payoff(pc.ARITH, 103.0, -1.0)]
    key = lambda r: (r.price, r.std_error, r.sum_payoff, r.sumsq_payoff, r.n_paths_done)  # noqa: E731
    res9, v9, _ = solve_path(hhlib, m, c, every, start, payoffs)
    assert len({key(r) for r in res9}) == 9
    for lo, hi in [(k, k + 1) for k in range(9)] + [(5, 9), (2, 7)]:
        res, v, _ = solve_path(hhlib, m, c, every, start, payoffs[lo:hi])
        for j, k in enumerate(range(lo, hi)):
            assert key(res[j]) == key(res9[k]), (lo, hi, k)
            np.testing.assert_array_equal(v[j], v9[k])


# ---- (e) closed forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("every", [1, 3])
def test_closed_forms_under_lognormal_dynamics(hhlib, every):
    """The Euler step on the log state is the exact lognormal transition: no discretisation bias, every price within 4
    of its own standard errors of the closed form (fixed seeds)."""
    S0 = K = 100.0
    r, sigma, T, steps, n = 0.05, 0.25, 0.75, 12, 200_000
    m = _ffi.make_model(S0=S0, sigma=sigma, r=r, T=T)
    c = config(LOGN, n, steps, 0)
    payoffs = [pc.payoff(pc.GEOM, K, 1.0), pc.payoff(pc.GEOM, K, -1.0), pc.payoff(pc.DCASH, K, 1.0, cash=3.0),
               pc.payoff(pc.DCASH, K, -1.0, cash=3.0), pc.payoff(pc.DASSET, K, 1.0), pc.payoff(pc.DASSET, K, -1.0)]
    exact = [pc.geometric_asian(S0, K, r, sigma, T, steps, every, True, 1.0), pc.geometric_asian(S0, K, r, sigma, T, steps, every, True, -1.0),
             pc.digital_cash(S0, K, r, sigma, T, 3.0, 1.0), pc.digital_cash(S0, K, r, sigma, T, 3.0, -1.0),
             pc.digital_asset(S0, K, r, sigma, T, 1.0), pc.digital_asset(S0, K, r, sigma, T, -1.0)]
    K_ = len(payoffs)
    arr, res = (_ffi.hh_path_payoff * K_)(*payoffs), (_ffi.hh_result * K_)()
    hhlib.check(hhlib.lib.hh_mc_solve_path(hhlib.handle, C.byref(m), C.byref(c), every, 1, arr, K_, res, None, None))
    for k in range(K_):
        z = (res[k].price - exact[k]) / res[k].std_error
        print(f"\nclosed form, every={every} payoff {k}: price {res[k].price:.6f} exact {exact[k]:.6f} z {z:+.2f}")
        assert abs(z) <= 4.0, (k, res[k].price, exact[k], z)


# ---- (f) argument errors ---------------------------------------------------------------------------------------------

def error_rows():
    r = []
    one = lambda **kw: [pc.payoff(**{**dict(kind=pc.ARITH), **kw})]  # noqa: E731

    def add(i, code, text, cfg=None, every=2, payoffs=None, n_payoffs=None, null=None, stats_only=False):
        r.append(dict(id=i, code=code, text=text, cfg=cfg or {}, every=every, payoffs=payoffs, n_payoffs=n_payoffs, null=null,
                      stats_only=stats_only))

    who = "hh_mc_solve_path"
    for null in ("model", "cfg", "payoffs", "out"):
        add("null." + null, INV, who + ": NULL argument", null=null)
    add("replay", UNS, who + ": GENERATE noise, no dual partials", cfg=dict(noise_mode=_ffi.HH_NOISE_REPLAY))
    add("partials", UNS, who + ": GENERATE noise, no dual partials", cfg=dict(n_partials=1))
    add("exact_law", UNS, who + " needs LognormalDynamics or HestonDynamics + EulerMaruyama", cfg=dict(dyn=LOGN, strat=_ffi.HH_EXACT_LAW))
    add("broadie_kaya", UNS, who + " needs LognormalDynamics or HestonDynamics + EulerMaruyama", cfg=dict(strat=_ffi.HH_BROADIE_KAYA))
    add("every.zero", INV, who + ": monitor_every (0) must be >= 1 and divide n_steps (4)", every=0)
    add("every.divisor", INV, who + ": monitor_every (3) must be >= 1 and divide n_steps (4)", every=3)
    add("every.beyond", INV, who + ": monitor_every (8) must be >= 1 and divide n_steps (4)", every=8)
    add("n_payoffs.zero", INV, who + ": 1 .. 1024 payoffs", n_payoffs=0)
    add("n_payoffs.max", INV, who + ": 1 .. 1024 payoffs", n_payoffs=1025)
    add("kind", INV, who + ": payoff 0: unknown kind 6", payoffs=one(kind=6))
    add("kind.negative", INV, who + ": payoff 1: unknown kind -1", payoffs=one() + one(kind=-1))
    add("barrier_type", INV, who + ": payoff 0: unknown barrier type 4", payoffs=one(kind=pc.BARRIER, barrier_type=4, barrier=1.0))
    add("cp", INV, who + ": payoff 0: cp must be +1 or -1", payoffs=one(cp=0.5))
    for f in ("strike", "rebate", "cash"):
        for bad in (math.inf, math.nan):
            add(f"{f}.{bad}", INV, who + ": payoff 0: strike, rebate, cash finite; barrier not NaN", payoffs=one(**{f: bad}))
    add("barrier.nan", INV, who + ": payoff 0: strike, rebate, cash finite; barrier not NaN", payoffs=one(kind=pc.BARRIER, barrier=math.nan))
    add("stats.null", INV, "hh_mc_path_stats: NULL argument", null="stats", stats_only=True)
    add("stats.every", INV, "hh_mc_path_stats: monitor_every (3) must be >= 1 and divide n_steps (4)", every=3, stats_only=True)
    add("stats.replay", UNS, "hh_mc_path_stats: GENERATE noise, no dual partials", cfg=dict(noise_mode=_ffi.HH_NOISE_REPLAY), stats_only=True)
    return r


def test_argument_errors_leave_the_context_usable():
    ctx = _ffi.Context(0)
    try:
        n, steps = 10, 4
        seeds = seeds_for(n)
        host = np.zeros(_ffi.HH_PATH_STATS * n)
        out = (_ffi.hh_result * 2)()
        good = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.ARITH))
        m = _ffi.make_model()
        for row in error_rows():
            kw = dict(row["cfg"])
            c = _ffi.make_config(kw.pop("dyn", HEST), kw.pop("strat", EULER), n, steps, seeds=seeds, **kw)
            if c.noise_mode == _ffi.HH_NOISE_REPLAY:
                c.replay, c.replay_len = host.ctypes.data, host.size
            null = row["null"]
            pm, pcfg = (None if null == "model" else C.byref(m)), (None if null == "cfg" else C.byref(c))
            if row["stats_only"]:
                rc = ctx.lib.hh_mc_path_stats(ctx.handle, pm, pcfg, row["every"], 0, None if null == "stats" else host.ctypes.data, 0, None)
            else:
                ps = row["payoffs"]
                arr = (_ffi.hh_path_payoff * len(ps))(*ps) if ps else good
                k = row["n_payoffs"] if row["n_payoffs"] is not None else len(arr)
                rc = ctx.lib.hh_mc_solve_path(ctx.handle, pm, pcfg, row["every"], 0, None if null == "payoffs" else arr, k,
                                              None if null == "out" else out, None, None)
            assert rc == row["code"], (row["id"], rc)
            assert ctx.lib.hh_last_error(ctx.handle).decode() == row["text"], row["id"]
            # the context still solves
            c = _ffi.make_config(HEST, EULER, n, steps, seeds=seeds)
            ctx.check(ctx.lib.hh_mc_solve_path(ctx.handle, C.byref(m), C.byref(c), 2, 0, good, 1, out, None, None))
            assert out[0].price > 0.0 and out[0].n_paths_done == n
        # a barrier may be infinite
        inf = (_ffi.hh_path_payoff * 2)(pc.payoff(pc.BARRIER, barrier_type=pc.UP_OUT, barrier=math.inf),
                                        pc.payoff(pc.BARRIER, barrier_type=pc.DOWN_IN, barrier=-math.inf, rebate=1.0))
        ctx.check(ctx.lib.hh_mc_solve_path(ctx.handle, C.byref(m), C.byref(c), 2, 0, inf, 2, out, None, None))
        assert out[0].price > 0.0 and out[1].price == pytest.approx(m.discount)
    finally:
        ctx.close()


# ---- (g) the Python layer --------------------------------------------------------------------------------------------

REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


def python_payoffs():
    m3 = hh.Monitoring(3, True)
    return [hh.AsianOption(100.0, EXP, hh.Call(), hh.ArithmeticAverage(), m3),
            hh.AsianOption(100.0, EXP, hh.Put(), hh.GeometricAverage(), m3),
            hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), rebate=1.0, monitoring=m3),
            hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndIn(), rebate=1.0, monitoring=m3),
            hh.BarrierOption(100.0, 90.0, EXP, hh.Put(), hh.DownAndOut(), monitoring=m3),
            hh.BarrierOption(100.0, 90.0, EXP, hh.Put(), hh.DownAndIn(), monitoring=m3),
            hh.DigitalOption(100.0, EXP, hh.Call(), hh.CashOrNothing(5.0)),
            hh.DigitalOption(100.0, EXP, hh.Put(), hh.AssetOrNothing())]


@pytest.mark.parametrize("anti", [False, True])
def test_solve_on_each_payoff_type_is_the_cabi_result(hhlib, anti):
    from hedgehog_jl_amd.montecarlo import _path_structs, pack_path_payoff
    mkt = hh.HestonInputs(REF, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    cfg = hh.SimulationConfig(700, steps=12, seeds=seeds_for(700), variance_reduction=hh.Antithetic() if anti else hh.NoVarianceReduction())
    mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    for p in python_payoffs():
        sol = hh.solve(hh.PricingProblem(p, mkt), mc)
        model, c, every, start, _ = _path_structs([p], mkt, mc)
        assert (every, start) == ((3, True) if hasattr(p, "monitoring") else (12, False))
        c.seeds, c.seeds_len = cfg.seeds.ctypes.data, cfg.seeds.size
        res, _, stats = solve_path(hhlib, model, c, every, int(start), [pack_path_payoff(p)])
        assert (sol.price, sol.std_error) == (res[0].price, res[0].std_error) and sol.price > 0.0
        assert sol.ensemble.shape == (5, 1400 if anti else 700)
        np.testing.assert_array_equal(sol.ensemble, stats)
        assert hh.solve(hh.PricingProblem(p, mkt), mc, ensemble=False).ensemble is None


def test_a_mixed_basket_is_its_single_solves(hhlib):
    mkt = hh.HestonInputs(REF, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    n = 700
    cfg = hh.SimulationConfig(n, steps=12, seeds=seeds_for(n), variance_reduction=hh.Antithetic())
    mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
    vanilla = hh.VanillaOption(100.0, EXP, hh.European(), hh.Call(), hh.Spot())
    daily = hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=hh.Monitoring(1))
    payoffs = python_payoffs() + [vanilla, daily]
    basket = hh.solve(hh.BasketPricingProblem(payoffs, mkt), mc)
    assert len(basket.solutions) == len(payoffs)
    for p, sol in zip(payoffs, basket.solutions):
        single = hh.solve(hh.PricingProblem(p, mkt), mc, ensemble=False)
        assert sol.problem.payoff is p and sol.ensemble is None
        if p is vanilla:  # alone it is the European solve: the same samples summed in another order
            d = (n - 1) * U * single.result.sum_payoff
            assert abs(sol.result.sum_payoff - single.result.sum_payoff) <= d
            assert abs(sol.price - single.price) <= single.result.price / single.result.sum_payoff * d + np.spacing(single.price)
        else:
            assert (sol.price, sol.std_error) == (single.price, single.std_error), p
    # the knock-out and the knock-in of a pair add up to the vanilla and the rebate, to the sums' rounding
    out_, in_, van = basket.solutions[2].price, basket.solutions[3].price, basket.solutions[8].price
    assert out_ + in_ == pytest.approx(van + 1.0 * math.exp(-0.03), rel=1e-12)


def test_a_finite_difference_delta_is_its_two_solves(hhlib):
    mkt = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    cfg = hh.SimulationConfig(700, steps=12, seeds=seeds_for(700))
    mc = hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg)
    asian = hh.AsianOption(100.0, EXP, hh.Call(), hh.ArithmeticAverage(), hh.Monitoring(3))
    prob, eps = hh.PricingProblem(asian, mkt), 1e-2
    delta = hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.FiniteDifference(eps), mc).greek
    up = hh.solve(hh.set(prob, hh.SpotLens(), 100.0 * (1 + eps)), mc).price
    down = hh.solve(hh.set(prob, hh.SpotLens(), 100.0 * (1 - eps)), mc).price
    assert delta == (up - down) / (2 * eps * 100.0) and 0.3 < delta < 0.8
