"""Local volatility on a tabulated surface on the device (hh_localvol.hip) — hh_mc_path_stats_lv, hh_mc_solve_path_lv and
the Python route above them.

  * PATH BY PATH against the restatement of tests/localvol_cases.py at 50 digits on the draws the device makes itself
    (the oracle's host Philox, the normals restated by hh_rng.h's formulas): every row of every member within
    euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A).  257 trajectories (two workgroups, a one-lane tail), on 1, 3
    and 12 steps; tables of (1, 2), (2, 3), (5, 33) nodes — the last so narrow that states leave the grid on both sides,
    with times that start after 0 and end before T — the full 64 KiB (32, 256) and a row of 8192.  257 on 3 steps is the
    smallest case in which the tail workgroup, the odd step count (one Philox block feeds two steps) and the table load
    all occur; a wrong row, cell or weight moves a state by far more than a bar.
  * IDENTITIES, bit for bit: a constant table gives hh_mc_path_stats_ex's rows under sigma = σ0; five equal rows give the
    one-row table's; trajectory i does not depend on the size of the call; a payoff's result does not depend on its
    neighbours; path_values are the payoffs of the returned statistics.
  * THE LAW, fixed seeds, 2¹⁸ trajectories, 64 steps, T = 1: the martingale; Black–Scholes on a table that varies in
    time only; the CEV model's closed form on its analytic table and on the table Dupire's formula makes of the
    fixture's prices; the bridge rows against the monitored ones.
  * Errors: every HH_ERR_INVALID / HH_ERR_UNSUPPORTED case of the header, with its text, without a launch.
The module prints its worst error/bar per row at its end (`-s`)."""
import ctypes as C
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from hedgehog_jl_amd import localvol as hlv  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import localvol_cases as lc  # noqa: E402
from tests import path_bridge_cases as bc  # noqa: E402
from tests import path_payoff_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

MONITORED, BRIDGE = _ffi.HH_EXTREMES_MONITORED, _ffi.HH_EXTREMES_BRIDGE
ROWS = {MONITORED: _ffi.HH_PATH_STATS, BRIDGE: _ffi.HH_PATH_STATS_BRIDGE}
ROW_NAMES = ("SUM_S", "SUM_X", "MAX_S", "MIN_S", "S_T", "CMAX_S", "CMIN_S")
_cache = {}


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("local volatility (device)")
    yield w
    w.report()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def path_stats(ctx, m, lv, c, every, start, extremes):
    stats = np.empty((ROWS[extremes], n_total(c)))
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_lv(ctx.handle, C.byref(m), C.byref(lv), C.byref(c), every, start, extremes,
                                          stats.ctypes.data, 0, C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return stats


def solve_path(ctx, m, lv, c, every, start, extremes, payoffs, want=True):
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = (np.empty((K, n_total(c))), np.empty((ROWS[extremes], n_total(c)))) if want else (None, None)
    ctx.check(ctx.lib.hh_mc_solve_path_lv(ctx.handle, C.byref(m), C.byref(lv), C.byref(c), every, start, extremes, arr, K, res,
                                          values.ctypes.data if want else None, stats.ctypes.data if want else None))
    return list(res), values, stats


def lognormal_stats(ctx, m, c, every, start, extremes):
    stats = np.empty((ROWS[extremes], n_total(c)))
    ctx.check(ctx.lib.hh_mc_path_stats_ex(ctx.handle, C.byref(m), C.byref(c), every, start, extremes, stats.ctypes.data, 0, None))
    return stats


def same_result(a, b):
    return (a.price, a.std_error, a.sum_payoff, a.sumsq_payoff, a.n_paths_done) == \
        (b.price, b.std_error, b.sum_payoff, b.sumsq_payoff, b.n_paths_done)


def law_seeds(n, salt=3):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt)


def payoff_list():
    return [pc.payoff(pc.VANILLA, 100.0, 1.0), pc.payoff(pc.ARITH, 98.0, 1.0), pc.payoff(pc.GEOM, 101.0, -1.0),
            pc.payoff(pc.BARRIER, 95.0, 1.0, pc.DOWN_OUT, 80.0, 1.5), pc.payoff(pc.DCASH, 102.0, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 99.0, -1.0), pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0),
            pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FIXED, 100.0, 1.0)]


# ---- (a) path by path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extremes", [MONITORED, BRIDGE], ids=["monitored", "bridge"])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("include_start", [0, 1])
@pytest.mark.parametrize("shape", lc.PATH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", lc.SURFACES)
def test_path_by_path(hhlib, oracle, worst, name, shape, include_start, anti, extremes):
    n_steps, every = shape
    surf, seeds = cached(("surf", name), lambda: lc.surface(name)), lc.path_seeds()
    Z = cached(("Z", n_steps), lambda: lc.step_normals(oracle, seeds, n_steps))
    U = cached(("U", n_steps), lambda: lc.bridge_uniforms(oracle, seeds, n_steps))
    ref = cached(("ref", name, shape, include_start), lambda: lc.reference(lc.MODEL, surf, n_steps, Z, U, 1, every, include_start))
    if name == "narrow" and n_steps > 1:  # steps clamped below, above and inside the grid (counted on the fp64 restatement)
        assert all(ref["counts"].get(k, 0) > 0 for k in (-1, 0, 1)), ref["counts"]
    bars = etc.path_bar(ref["e64"], ref["A"])
    got = path_stats(hhlib, lc.model_of(), lc.localvol_of(surf), lc.config_of(lc.PATH_N, n_steps, seeds, anti), every,
                     include_start, extremes)
    bad = []
    for mem in range(2 if anti else 1):
        for i in range(lc.PATH_N):
            for row in range(ROWS[extremes]):
                bad.append(worst.check(ROW_NAMES[row], got[row][mem * lc.PATH_N + i], ref["want"][mem][i][row], bars[mem][i][row],
                                       f"{name} {n_steps}x{every} start={include_start} anti={anti} extremes={extremes} "
                                       f"member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ---- (b) identities, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extremes", [MONITORED, BRIDGE], ids=["monitored", "bridge"])
@pytest.mark.parametrize("anti", [0, 1])
def test_constant_table_is_the_lognormal_kernel(hhlib, anti, extremes):
    """every entry σ0: hh_mc_path_stats_ex's rows under model->sigma = σ0, all of them, in both forms"""
    s0, n, steps = 0.2718281828, 513, 5
    seeds = law_seeds(n, 41)
    surf = dict(times=np.array([0.2, 0.6, 0.9]), vols=np.full((3, 9), s0), x_lo=lc.X0 - 0.1, h=0.025)
    c = lc.config_of(n, steps, seeds, anti)
    got = path_stats(hhlib, lc.model_of(), lc.localvol_of(surf), c, 1, 1, extremes)
    want = lognormal_stats(hhlib, lc.model_of(sigma=s0), c, 1, 1, extremes)
    assert got.shape[0] == ROWS[extremes] and np.array_equal(got, want)


@pytest.mark.parametrize("anti", [0, 1])
def test_five_equal_rows_are_the_one_row_table(hhlib, anti):
    n, steps = 300, 6
    row = lc.surface("narrow")["vols"][2:3]
    one = dict(times=np.array([0.4]), vols=row, x_lo=lc.X0 - 0.08, h=0.005)
    five = dict(times=np.array([0.1, 0.3, 0.5, 0.7, 0.9]), vols=np.repeat(row, 5, axis=0), x_lo=lc.X0 - 0.08, h=0.005)
    c = lc.config_of(n, steps, law_seeds(n, 43), anti)
    a = path_stats(hhlib, lc.model_of(), lc.localvol_of(one), c, 2, 0, BRIDGE)
    b = path_stats(hhlib, lc.model_of(), lc.localvol_of(five), c, 2, 0, BRIDGE)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


@pytest.mark.parametrize("anti", [0, 1])
def test_one_wave_and_many(hhlib, anti):
    """n_paths of 1, 63, 64, 65, 256 and 513 on 3 steps: trajectory i of every size == trajectory i of the largest"""
    big = 513
    seeds = law_seeds(big, 17)
    m, lv = lc.model_of(), lc.localvol_of(lc.surface("narrow"))
    whole = path_stats(hhlib, m, lv, lc.config_of(big, 3, seeds, anti), 1, 1, BRIDGE)
    assert np.all(np.isfinite(whole))
    for n in (1, 63, 64, 65, 256, 513):
        stats = path_stats(hhlib, m, lv, lc.config_of(n, 3, seeds[:n], anti), 1, 1, BRIDGE)
        for mem in range(2 if anti else 1):
            assert np.array_equal(stats[:, mem * n:(mem + 1) * n], whole[:, mem * big:mem * big + n]), (n, mem)


@pytest.mark.parametrize("extremes", [MONITORED, BRIDGE], ids=["monitored", "bridge"])
def test_payoff_independence_and_path_values(hhlib, extremes):
    """result k of a 16-payoff call == the one-payoff call; path_values rows == the payoffs of the returned statistics"""
    n, n_steps, every, start = 3000, 6, 2, 1
    m, lv = lc.model_of(), lc.localvol_of(lc.surface("two_by_3"))
    c = lc.config_of(n, n_steps, law_seeds(n, 29), 1)
    payoffs = payoff_list() + [pc.payoff(pc.VANILLA, 70.0 + 10.0 * k, 1.0 if k % 2 else -1.0) for k in range(8)]
    assert len(payoffs) == 16
    together, values, stats = solve_path(hhlib, m, lv, c, every, start, extremes, payoffs)
    assert np.array_equal(path_stats(hhlib, m, lv, c, every, start, extremes), stats)
    n_mon = pc.n_mon(n_steps, every, start)
    for k, p in enumerate(payoffs):
        alone, _, _ = solve_path(hhlib, m, lv, c, every, start, extremes, [p], want=False)
        assert same_result(alone[0], together[k]), k
        want = bc.payoff_from_stats(stats, p, n_mon, extremes)
        if p.kind == pc.GEOM:  # numpy's exp against the device's
            np.testing.assert_allclose(values[k], want, rtol=1e-14, atol=1e-13)
        else:
            assert np.array_equal(values[k], want), k
        pair = (values[k][:n] + values[k][n:]) / 2
        assert together[k].sum_payoff == pytest.approx(math.fsum(pair), rel=1e-13, abs=1e-12)
        assert together[k].n_paths_done == n


# ---- (c) the law -----------------------------------------------------------------------------------------------------------

N_LAW, LAW_STEPS = 2 ** 18, 64
STRIKES = (80.0, 100.0, 120.0)


def cev_table():
    """the analytic table: σ0·(S/S0)^{β−1} on 257 nodes over log S0 ± 1.5, one row"""
    x = lc.X0 - 1.5 + 3.0 / 256 * np.arange(257)
    return dict(times=np.array([0.0]), vols=lc.cev_sigma(np.exp(x))[None, :], x_lo=lc.X0 - 1.5, h=3.0 / 256)


def cev_closed_form():
    with mp.workdps(30):
        return [float(lc.cev_call(1.0, K)) for K in STRIKES]


def cev_model():
    return lc.model_of(dict(S0=lc.CEV["S0"], r_drift=lc.CEV["r"], T=1.0))


def calls_on(ctx, surf, salt):
    c = lc.config_of(N_LAW, LAW_STEPS, law_seeds(N_LAW, salt))
    res, _, _ = solve_path(ctx, cev_model(), lc.localvol_of(surf), c, LAW_STEPS, 0, MONITORED,
                           [pc.payoff(pc.VANILLA, K, 1.0) for K in STRIKES], want=False)
    return res, c


def test_the_discounted_spot_is_a_martingale(hhlib):
    """e^{−rT}·mean S_T within 4 standard errors of S0, on the CEV table"""
    c = lc.config_of(N_LAW, LAW_STEPS, law_seeds(N_LAW, 5))
    S = path_stats(hhlib, cev_model(), lc.localvol_of(cev_table()), c, LAW_STEPS, 0, MONITORED)[pc.S_T]
    D = math.exp(-lc.CEV["r"])
    miss = (D * S.mean() - lc.CEV["S0"]) / (D * S.std(ddof=1) / math.sqrt(N_LAW))
    print(f"\ne^-rT mean S_T {D * S.mean():.4f}: {miss:+.2f} standard errors from S0")
    assert abs(miss) <= 4.0


def test_time_only_table_is_black_scholes_on_its_variance(hhlib):
    """σ(t) alone: the log-Euler step is exact in law, so the call is Black–Scholes' on Σ_k σ(t_k)²·dt, summed here"""
    sig = np.array([0.15, 0.35, 0.2, 0.3])
    surf = dict(times=np.array([0.1, 0.4, 0.6, 0.9]), vols=np.repeat(sig[:, None], 2, axis=1), x_lo=lc.X0 - 1.0, h=2.0)
    dt = 1.0 / LAW_STEPS
    var = sum(lc.get_sigma(surf, float(k) * dt, lc.X0) ** 2 * dt for k in range(LAW_STEPS))
    assert 0.15 ** 2 < var < 0.35 ** 2
    want = bc.bs_call(100.0, 100.0, 0.03, math.sqrt(var), 1.0)
    c = lc.config_of(N_LAW, LAW_STEPS, law_seeds(N_LAW, 7))
    res, _, _ = solve_path(hhlib, lc.model_of(), lc.localvol_of(surf), c, LAW_STEPS, 0, MONITORED,
                           [pc.payoff(pc.VANILLA, 100.0, 1.0)], want=False)
    miss = (res[0].price - want) / res[0].std_error
    print(f"\ntime-only table: price {res[0].price:.5f}, Black–Scholes {want:.5f}, {miss:+.2f} standard errors of {res[0].std_error:.4f}")
    assert res[0].std_error > 0.0 and abs(miss) <= 4.0


def test_the_law_against_the_cev_closed_form(hhlib):
    """calls at K = 80, 100, 120 on the analytic CEV table within 4 standard errors of Schroder's closed form; the flat-σ0
    solve on the same seeds more than 6 away at K = 80 and K = 120"""
    want = cev_closed_form()
    res, c = calls_on(hhlib, cev_table(), 9)
    for r, w, K in zip(res, want, STRIKES):
        miss = (r.price - w) / r.std_error
        print(f"\nlocal vol K={K:g}: price {r.price:.5f}, closed form {w:.5f}, {miss:+.2f} standard errors of {r.std_error:.4f}")
        assert r.std_error > 0.0 and abs(miss) <= 4.0, (K, r.price, w, r.std_error)
    flat_m = lc.model_of(dict(S0=100.0, r_drift=lc.CEV["r"], T=1.0), sigma=lc.CEV["sigma0"])
    arr, out = (_ffi.hh_path_payoff * 3)(*[pc.payoff(pc.VANILLA, K, 1.0) for K in STRIKES]), (_ffi.hh_result * 3)()
    hhlib.check(hhlib.lib.hh_mc_solve_path_ex(hhlib.handle, C.byref(flat_m), C.byref(c), LAW_STEPS, 0, MONITORED, arr, 3, out, None, None))
    for k in (0, 2):
        miss = (out[k].price - want[k]) / out[k].std_error
        print(f"\nflat sigma0 K={STRIKES[k]:g}: price {out[k].price:.5f}, {miss:+.2f} standard errors")
        assert abs(miss) > 6.0


def test_the_law_on_the_dupire_table_of_the_fixture(hhlib):
    """the same three calls on the table dupire_local_vol makes of the fixture's fine grid: within 4 standard errors"""
    doc = lc.load_golden()
    fine = doc["fine"]
    s = hlv.dupire_local_vol(lambda T, K: fine.reshape(-1), doc["times"], doc["x_lo"], doc["x_hi"], doc["n_x"], lc.CEV["r"],
                             0.01, 0.005, vol_bounds=(0.02, 1.5), spot=lc.CEV["S0"])
    surf = dict(times=s.times, vols=s.vols, x_lo=s.x_lo, h=s.h)
    res, _ = calls_on(hhlib, surf, 13)
    for r, w, K in zip(res, cev_closed_form(), STRIKES):
        miss = (r.price - w) / r.std_error
        print(f"\nDupire table K={K:g}: price {r.price:.5f}, closed form {w:.5f}, {miss:+.2f} standard errors of {r.std_error:.4f}")
        assert r.std_error > 0.0 and abs(miss) <= 4.0, (K, r.price, w, r.std_error)


def test_bridge_extremes_contain_the_monitored_ones(hhlib):
    n = 2 ** 14
    c = lc.config_of(n, 16, law_seeds(n, 19), 1)
    st = path_stats(hhlib, cev_model(), lc.localvol_of(cev_table()), c, 4, 1, BRIDGE)
    assert np.all(st[_ffi.HH_STAT_CMAX_S] >= st[pc.MAX_S]) and np.all(st[_ffi.HH_STAT_CMIN_S] <= st[pc.MIN_S])
    assert np.any(st[_ffi.HH_STAT_CMAX_S] > st[pc.MAX_S]) and np.all(st[_ffi.HH_STAT_CMIN_S] > 0.0)


# ---- (d) errors ------------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")


def test_errors_come_back_without_a_launch(hhlib):
    ctx = hhlib
    n, steps = 300, 4
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    good_m = lc.model_of()
    base = lc.surface("two_by_3")
    good = lc.localvol_of(base)
    outs = (_ffi.hh_result * 1)()
    pay = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.VANILLA, 100.0, 1.0))
    stats = np.empty((7, n))
    cfg = lambda **kw: lc.config_of(n, steps, seeds, **kw)  # noqa: E731

    def both(mm, ll, cc, every=1, extremes=MONITORED, payoffs=pay):
        a = ctx.lib.hh_mc_solve_path_lv(ctx.handle, mm, ll, cc, every, 0, extremes, payoffs, 1, outs, None, None)
        ta = ctx.lib.hh_last_error(ctx.handle).decode()
        b = ctx.lib.hh_mc_path_stats_lv(ctx.handle, mm, ll, cc, every, 0, extremes, stats.ctypes.data, 0, None)
        return (a, ta), (b, ctx.lib.hh_last_error(ctx.handle).decode())

    def expect(mm, ll, cc, code, text, **kw):
        for who, (rc, msg) in zip(("hh_mc_solve_path_lv", "hh_mc_path_stats_lv"), both(mm, ll, cc, **kw)):
            assert rc == code and text in msg and who in msg, (who, rc, code, text, msg)

    def lv_of(**kw):
        d = dict(base, **kw)
        return lc.localvol_of(d)

    def with_fields(**kw):
        lv = lc.localvol_of(base)
        for k, v in kw.items():
            setattr(lv, k, v)
        return lv

    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
        m, c = C.byref(good_m), C.byref(cfg())
        expect(m, None, c, INV, "NULL argument")
        expect(None, C.byref(good), c, INV, "NULL argument")
        expect(m, C.byref(good), None, INV, "NULL argument")
        expect(m, C.byref(with_fields(times=None)), c, INV, "NULL argument")
        expect(m, C.byref(with_fields(vols=None)), c, INV, "NULL argument")
        expect(m, C.byref(with_fields(n_times=0)), c, INV, "n_times >= 1 and n_x >= 2")
        expect(m, C.byref(with_fields(n_x=1)), c, INV, "n_times >= 1 and n_x >= 2")
        big = dict(times=np.arange(1, 34) * 0.01, vols=np.full((33, 256), 0.2), x_lo=4.0, h=0.01)
        expect(m, C.byref(lc.localvol_of(big)), c, INV, "is above HH_LV_MAX_NODES")
        for times in ([NAN, 0.5], [0.25, INF], [-0.1, 0.5], [0.5, 0.5], [0.5, 0.25]):
            expect(m, C.byref(lv_of(times=np.array(times))), c, INV, "times")
        for bad in (0.0, -0.2, NAN, INF):
            v = base["vols"].copy()
            v[1, 2] = bad
            expect(m, C.byref(lv_of(vols=v)), c, INV, "vols[1][2] must be finite and > 0")
        for x_lo in (NAN, INF):
            expect(m, C.byref(lv_of(x_lo=x_lo)), c, INV, "x_lo must be finite")
        for h in (0.0, -0.5, NAN, INF):
            expect(m, C.byref(lv_of(h=h)), c, INV, "h must be finite and > 0")
        for d in (dict(S0=-1.0), dict(T=0.0), dict(T=INF), dict(r_drift=NAN)):
            expect(C.byref(lc.model_of(dict(lc.MODEL, **d))), C.byref(good), c, INV, "model scalars finite")
        expect(m, C.byref(good), c, INV, "must be >= 1 and divide n_steps", every=3)
        expect(m, C.byref(good), c, INV, "unknown extremes", extremes=2)
        expect(m, C.byref(good), C.byref(lc.config_of(0, steps, seeds)), INV, "1 <= n_paths")
        rc = ctx.lib.hh_mc_solve_path_lv(ctx.handle, m, C.byref(good), c, 1, 0, MONITORED,
                                         (_ffi.hh_path_payoff * 1)(pc.payoff(8, 100.0, 1.0)), 1, outs, None, None)
        assert rc == INV and "unknown kind" in ctx.lib.hh_last_error(ctx.handle).decode()
        for dyn, strat in ((_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA), (_ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW),
                           (_ffi.HH_HESTON, _ffi.HH_QE), (_ffi.HH_LOGNORMAL, _ffi.HH_BROADIE_KAYA)):
            expect(m, C.byref(good), C.byref(_ffi.make_config(dyn, strat, n, steps, seeds=seeds)), UNS,
                   "needs LognormalDynamics + EulerMaruyama")
        expect(m, C.byref(good), C.byref(cfg(noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4))), UNS, "GENERATE noise, no dual partials")
        expect(m, C.byref(good), C.byref(cfg(n_partials=2)), UNS, "GENERATE noise, no dual partials")
        assert ctx.read_timings() == []  # nothing was launched
        # model->sigma is not read: NaN above, anything here; the edges are admitted, and the context solves
        for sigma in (NAN, -3.0, 0.0):
            res, _, st = solve_path(ctx, lc.model_of(sigma=sigma), good, cfg(), 2, 1, BRIDGE, [pc.payoff(pc.VANILLA, 100.0, 1.0)])
            assert np.all(np.isfinite(st)) and res[0].price > 0.0 and res[0].n_paths_done == n
        cap = lc.localvol_of(lc.surface("cap"))
        assert np.all(np.isfinite(path_stats(ctx, good_m, cap, cfg(anti=1), 1, 0, MONITORED)))
        assert len(ctx.read_timings()) == 7  # two slots per solve, one for the statistics alone
    finally:
        ctx.enable_timing(False)


# ---- (e) the Python route --------------------------------------------------------------------------------------------------

def test_python_route_gives_the_c_calls_numbers(hhlib):
    ref, exp_ = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
    T = hh.yearfrac(ref, exp_)
    x = lc.X0 - 1.0 + 2.0 / 64 * np.arange(65)
    s = hh.LocalVolSurface([0.25, 0.75], x, np.vstack([lc.cev_sigma(np.exp(x)), 1.1 * lc.cev_sigma(np.exp(x))]))
    mkt = hh.LocalVolInputs(ref, 0.03, 100.0, s)
    surf = dict(times=s.times, vols=s.vols, x_lo=s.x_lo, h=s.h)
    n, steps = 4096, 12
    seeds = law_seeds(n, 23)
    for anti in (False, True):
        vr = hh.Antithetic() if anti else hh.NoVarianceReduction()
        method = hh.MonteCarlo(hh.LocalVolDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=vr))
        vanilla = hh.VanillaOption(105.0, exp_, hh.European(), hh.Call(), hh.Spot())
        asian = hh.AsianOption(100.0, exp_, hh.Call(), monitoring=hh.Monitoring(3))
        out = hh.BarrierOption(100.0, 130.0, exp_, hh.Call(), hh.UpAndOut(), monitoring=hh.ContinuousMonitoring())
        look = hh.LookbackOption(exp_, hh.Call(), monitoring=hh.Monitoring(3))
        m = lc.model_of(dict(S0=100.0, r_drift=0.03, T=T))
        c = lc.config_of(n, steps, seeds, int(anti))
        for payoff, packed, every, ext in ((vanilla, pc.payoff(pc.VANILLA, 105.0, 1.0), steps, MONITORED),
                                           (asian, pc.payoff(pc.ARITH, 100.0, 1.0), 3, MONITORED),
                                           (out, pc.payoff(pc.BARRIER, 100.0, 1.0, pc.UP_OUT, 130.0, 0.0), steps, BRIDGE),
                                           (look, pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0), 3, MONITORED)):
            sol = hh.solve(hh.PricingProblem(payoff, mkt), method)
            res, _, stats = solve_path(hhlib, m, lc.localvol_of(surf), c, every, 0, ext, [packed])
            assert sol.price == res[0].price and sol.std_error == res[0].std_error and sol.price > 0.0, type(payoff).__name__
            assert np.array_equal(sol.ensemble, stats)
        basket = hh.solve(hh.BasketPricingProblem([asian, vanilla, out, look], mkt), method)
        for p, sol in zip((asian, vanilla, out, look), basket.solutions):
            assert sol.price == hh.solve(hh.PricingProblem(p, mkt), method).price
        fd = hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla, mkt), hh.SpotLens()), hh.FiniteDifference(1e-2), method)
        assert 0.2 < fd.greek < 0.8
