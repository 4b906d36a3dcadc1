"""Variance Gamma on the device (hh_vg.hip, hh_fourier.hip) — hh_mc_solve_vg, hh_mc_path_stats_vg, hh_mc_solve_path_vg,
hh_carr_madan_vg and the Python routes above them.

  * PATH BY PATH against the restatement of tests/vg_cases.py at 50 digits, on the draws the device makes itself: the
    attempts' normals and the Brownian normals are restated from the oracle's host Philox words by hh_rng.h's formulas.
    Every sample and statistic within euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A).  A wrong accept/reject
    decision at any attempt replaces the step's variate by another draw altogether: the bars catch it; the walk's attempt
    counts are those tests/golden/make_vg_exact.py recorded with their margins.
  * COMPOSITION, bit for bit: the terminal law shards by path_offset; a payoff's result does not depend on its neighbours.
  * THE LAW, fixed seeds: prices within 4 standard errors of the 50-digit mixing integral by the terminal law and by the
    path form on 1, 4 and 16 steps (an inexact step would break the equality across step counts); the matched-variance
    lognormal price lies more than 10 standard errors away, so the comparison has power.
  * Carr–Madan against the exactly integrated truncated integral.
  * Errors: every HH_ERR_INVALID / HH_ERR_UNSUPPORTED case of the header, with its text, without a launch.
The module prints its worst error/bar per kind of comparison at its end (`-s`)."""
import ctypes as C
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from hedgehog_jl_amd import montecarlo as hmc  # noqa: E402
from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import path_bridge_cases as bc  # noqa: E402
from tests import path_payoff_cases as pc  # noqa: E402
from tests import vg_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

DOC = vc.load_golden()
GBM, HEST, EXACT, EULER = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON, _ffi.HH_EXACT_LAW, _ffi.HH_EULER_MARUYAMA
MONITORED = _ffi.HH_EXTREMES_MONITORED
SEED = np.array([vc.TERMINAL_SEED], dtype=np.uint64)
_cache = {}


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("variance gamma (device)")
    yield w
    w.report()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- calls ---------------------------------------------------------------------------------------------------------------

def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def solve_vg(ctx, m, g, c, want_terminal=True):
    res = _ffi.hh_result()
    term = np.zeros(n_total(c)) if want_terminal else None
    ctx.check(ctx.lib.hh_mc_solve_vg(ctx.handle, C.byref(m), C.byref(g), C.byref(c), C.byref(res),
                                     term.ctypes.data if want_terminal else None))
    assert res.n_paths_done == c.n_paths and res.kernel_ms > 0.0
    return res, term


def path_stats_vg(ctx, m, g, c, every, start):
    stats = np.empty((_ffi.HH_PATH_STATS, n_total(c)))
    ctx.check(ctx.lib.hh_mc_path_stats_vg(ctx.handle, C.byref(m), C.byref(g), C.byref(c), every, start, stats.ctypes.data, 0, None))
    return stats


def solve_path_vg(ctx, m, g, c, every, start, payoffs, want=True):
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = (np.empty((K, n_total(c))), np.empty((_ffi.HH_PATH_STATS, n_total(c)))) if want else (None, None)
    ctx.check(ctx.lib.hh_mc_solve_path_vg(ctx.handle, C.byref(m), C.byref(g), C.byref(c), every, start, arr, K, res,
                                          values.ctypes.data if want else None, stats.ctypes.data if want else None))
    return list(res), values, stats


def same_result(a, b):
    return (a.price, a.std_error, a.sum_payoff, a.sumsq_payoff, a.n_paths_done) == \
        (b.price, b.std_error, b.sum_payoff, b.sumsq_payoff, b.n_paths_done)


def terminal_config(n, anti, offset=0, **kw):
    return _ffi.make_config(GBM, EXACT, n, 1, antithetic=anti, seeds=SEED, path_offset=offset, **kw)


def path_config(n, n_steps, anti, seeds, **kw):
    return _ffi.make_config(GBM, EXACT, n, n_steps, antithetic=anti, seeds=seeds, **kw)


# ---- 5. path by path -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("shape", vc.DEVICE_SHAPES)
def test_terminal_law_path_by_path(hhlib, oracle, worst, shape, anti):
    """257 and 513 trajectories — a partial tile and more than one — at shapes 0.008 (boosted, underflows), 0.25 (boosted)
    and 4.7: every sample within its bar, the mirrors at terminal[n + i], the sums those of the samples"""
    case = vc.shape_case(shape, 1)
    d = cached(("t", shape), lambda: vc.PathDraws(oracle, case, 1, vc.PATH_N, [vc.TERMINAL_SEED], terminal=True))
    rec = next(r for r in DOC["counts"]["terminal"] if r["shape"] == shape)
    assert [a[0] for a in d.attempts] == rec["attempts"] and d.margin >= vc.MARGIN
    ref = d.reference(anti, 1, 0)
    m, g = vc.model_of(case, 100.0, 1.0), vc.vg_of(case)
    bad = []
    for n in vc.PATH_SIZES:
        res, term = solve_vg(hhlib, m, g, terminal_config(n, anti))
        for mem in range(ref["members"]):
            for i in range(n):
                bad.append(worst.check("terminal mirror" if mem else "terminal", term[mem * n + i], ref["want"][mem][i][pc.S_T],
                                       ref["bars"][mem][i][pc.S_T], f"shape {shape} n={n} path {i}"))
        pay = np.maximum(term - 100.0, 0.0)
        pay = (pay[:n] + pay[n:]) / 2 if anti else pay
        assert res.sum_payoff == pytest.approx(math.fsum(pay), rel=1e-13, abs=1e-300)
        assert res.price == pytest.approx(m.discount * math.fsum(pay) / n, rel=1e-13, abs=1e-300)
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])
    print(f"\nterminal shape {shape} antithetic={anti}: worst error/bar so far {max(v[0] for v in worst.w.values()):.3g}")


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("n_steps", vc.PATH_STEPS)
@pytest.mark.parametrize("shape", vc.DEVICE_SHAPES)
def test_path_form_path_by_path(hhlib, oracle, worst, shape, n_steps, anti):
    """All five rows of 257 and of 513 trajectories for n_steps of 1, 5 (the odd tail of the two-step loop: a half-read
    block of normals) and 8, monitored at every step and at expiry alone, with and without the start"""
    seeds, case = vc.path_seeds(), vc.shape_case(shape, n_steps)
    d = cached(("p", shape, n_steps), lambda: vc.PathDraws(oracle, case, n_steps, vc.PATH_N, seeds))
    rec = next(r for r in DOC["counts"]["path"] if r["shape"] == shape and r["n_steps"] == n_steps)
    assert d.attempts == rec["attempts"] and d.margin >= vc.MARGIN
    m, g = vc.model_of(case), vc.vg_of(case)
    bad = []
    for every in sorted({1, n_steps}):
        for start in (0, 1):
            ref = d.reference(anti, every, start)
            for n in vc.PATH_SIZES:
                stats = path_stats_vg(hhlib, m, g, path_config(n, n_steps, anti, seeds[:n]), every, start)
                for mem in range(ref["members"]):
                    for i in range(n):
                        for row in range(5):
                            bad.append(worst.check(f"row {row}", stats[row][mem * n + i], ref["want"][mem][i][row],
                                                   ref["bars"][mem][i][row],
                                                   f"shape {shape} {n_steps}x{every} start={start} n={n} member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])
    print(f"\npath form shape {shape} {n_steps} steps antithetic={anti}: worst error/bar so far {max(v[0] for v in worst.w.values()):.3g}")


# ---- 6. composition --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
def test_terminal_law_composes(hhlib, anti):
    """[0, 513) is [0, 200) followed by [200, 513) with path_offset = 200, bit for bit; the same call gives the same bits"""
    n, k = 513, 200
    m, g = vc.model_of(vc.BASE, 105.0, 1.0), vc.vg_of(vc.BASE)
    res, whole = solve_vg(hhlib, m, g, terminal_config(n, anti))
    ra, a = solve_vg(hhlib, m, g, terminal_config(k, anti))
    rb, b = solve_vg(hhlib, m, g, terminal_config(n - k, anti, offset=k))
    assert np.array_equal(whole[:n], np.concatenate([a[:k], b[:n - k]]))
    if anti:
        assert np.array_equal(whole[n:], np.concatenate([a[k:], b[n - k:]]))
    assert len(set(whole[:n])) == n and np.all(whole > 0.0)
    assert res.sum_payoff == pytest.approx(ra.sum_payoff + rb.sum_payoff, rel=1e-13)
    again, _ = solve_vg(hhlib, m, g, terminal_config(n, anti), want_terminal=False)
    assert same_result(res, again)


# ---- 7. prices -------------------------------------------------------------------------------------------------------------

def within(res, want, what, bar=4.0):
    miss = abs(res.price - float(want)) / res.std_error
    print(f"\n{what}: price {res.price:.6f}, exact {float(want):.6f}, {miss:.2f} standard errors")
    assert res.std_error > 0.0 and miss <= bar, (what, res.price, float(want), res.std_error)
    return miss


def mixing(K):
    return mp.mpf(next(r for r in DOC["prices"] if r["params"] == list(vc.PARAMS[0]) and r["K"] == K and r["cp"] > 0)["price"])


def test_prices_against_the_mixing_integral(hhlib):
    """2¹⁸ trajectories at (σ, θ, ν) = (0.2, −0.3, 0.5), T = 1, r = 0.03, S0 = 100: calls at K = 80, 100, 120 by the
    terminal law and by the path form on 1, 4 and 16 steps, each within 4 of its own standard errors of the 50-digit
    mixing price; the Black–Scholes price at the matched total variance σ² + θ²ν lies more than 10 standard errors from
    the same solve at K = 100 and K = 120; the discounted mean of S_T within 4 standard errors of S0 (a wrong ω misses);
    ν = 1e-4 (shape 10⁴, no boost): the call at K = 100 within 4 standard errors of Black–Scholes at σ"""
    case, n = dict(vc.BASE, discount=math.exp(-vc.BASE["r_drift"] * vc.BASE["T"])), 2 ** 18
    g = vc.vg_of(case)
    matched = math.sqrt(case["sigma"] ** 2 + case["theta"] ** 2 * case["nu"])
    for K in vc.STRIKES:
        res, _ = solve_vg(hhlib, vc.model_of(case, K, 1.0), g, terminal_config(n, 0), want_terminal=False)
        within(res, mixing(K), f"terminal law K={K:g}")
        if K >= 100.0:
            away = abs(res.price - float(vc.black_scholes(case, K, 1.0, vol=matched))) / res.std_error
            print(f"matched-variance lognormal: {away:.1f} standard errors away")
            assert away > 10.0, (K, away)
    res, _ = solve_vg(hhlib, vc.model_of(case, 0.0, 1.0), g, terminal_config(n, 0), want_terminal=False)
    within(res, case["S0"], "discounted mean of S_T")
    seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
    payoffs = [pc.payoff(pc.VANILLA, K, 1.0) for K in vc.STRIKES]
    for n_steps in (1, 4, 16):
        res, _, _ = solve_path_vg(hhlib, vc.model_of(case), g, path_config(n, n_steps, 0, seeds), n_steps, 0, payoffs, want=False)
        for r, K in zip(res, vc.STRIKES):
            within(r, mixing(K), f"path form, {n_steps} steps, K={K:g}")
    thin = dict(case, nu=1e-4)
    res, _ = solve_vg(hhlib, vc.model_of(thin, 100.0, 1.0), vc.vg_of(thin), terminal_config(n, 0), want_terminal=False)
    within(res, vc.black_scholes(thin, 100.0, 1.0), "nu = 1e-4 against Black–Scholes")


# ---- 8. payoffs on the statistics ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
def test_payoffs_on_the_statistics(hhlib, anti):
    """every payoff kind on 513 trajectories × 8 steps against path_cases.payoff_from_stats on the returned statistics and
    against its own sums (the antithetic pair averaged first); a payoff alone gives what it gives in the basket; a mixed
    basket is its single solves"""
    n, n_steps, every, start = 513, 8, 2, 1
    seeds = vc.path_seeds()
    m, g = vc.model_of(vc.BASE), vc.vg_of(vc.BASE)
    c = path_config(n, n_steps, anti, seeds)
    payoffs = vc.payoff_list()
    res, values, stats = solve_path_vg(hhlib, m, g, c, every, start, payoffs)
    assert np.array_equal(stats, path_stats_vg(hhlib, m, g, c, every, start))
    assert np.all(stats[pc.MAX_S] >= stats[pc.S_T]) and np.all(stats[pc.MIN_S] <= stats[pc.S_T]) and np.all(stats[pc.MIN_S] > 0.0)
    n_mon = pc.n_mon(n_steps, every, start)
    for k, q in enumerate(payoffs):
        want = bc.payoff_from_stats(stats, q, n_mon, MONITORED)
        if q.kind == pc.GEOM:  # numpy's exp against the device's
            np.testing.assert_allclose(values[k], want, rtol=1e-14, atol=1e-13)
        else:
            assert np.array_equal(values[k], want), k
        pair = (values[k][:n] + values[k][n:]) / 2 if anti else values[k]
        assert res[k].sum_payoff == pytest.approx(math.fsum(pair), rel=1e-13, abs=1e-12)
        assert res[k].sumsq_payoff == pytest.approx(math.fsum(pair * pair), rel=1e-13, abs=1e-12)
        assert res[k].n_paths_done == n
        alone, _, _ = solve_path_vg(hhlib, m, g, c, every, start, [q], want=False)
        assert same_result(alone[0], res[k]), k
    mixed, _, _ = solve_path_vg(hhlib, m, g, c, every, start, payoffs[::-1], want=False)
    assert all(same_result(a, b) for a, b in zip(mixed, res[::-1]))


# ---- 9. Carr–Madan ---------------------------------------------------------------------------------------------------------

def cm_arrays(rec):
    model, rows = rec["model"], rec["payoffs"]
    Ts = np.array([p["T"] for p in rows])
    return (np.array([p["K"] for p in rows]), np.array([p["cp"] for p in rows]), Ts, np.full(len(rows), model["r_drift"]),
            np.array([math.exp(-model["r_drift"] * T) for T in Ts]))


@pytest.mark.parametrize("name", ["set0", "set1", "set2", "tail"])
def test_carr_madan_against_the_exact_integral(hhlib, worst, name):
    """the three parameter sets at α = 1.5, bound 32, calls and puts at K = 80, 100, 120: every price against the exactly
    integrated truncated integral of the fixture within vg_cases.cm_bar — max(1e-14·S0, 20·e64, the power's own term);
    `tail`: the third set at bound 200, where what the truncation leaves out is below 1e-10·S0 — the device price within
    1e-10·S0 of the mixing price.  Measured maximum of error/bar: printed with the module's report."""
    rec = next(b for b in DOC["carr_madan"] if b["id"] == name)
    model, arrs, n = rec["model"], cm_arrays(rec), len(rec["payoffs"])
    m, g, out = vc.model_of(model), vc.vg_of(model), np.empty(n)
    hhlib.check(hhlib.lib.hh_carr_madan_vg(hhlib.handle, C.byref(m), C.byref(g), rec["alpha"], rec["bound"],
                                           *[a.ctypes.data for a in arrs], n, out.ctypes.data))
    bad = []
    for k, p in enumerate(rec["payoffs"]):
        case = cl.cm_case(dict(model, T=p["T"]), p["K"], rec["alpha"], rec["bound"], p["cp"])
        assert case["discount"] == arrs[4][k]
        bad.append(worst.check("carr-madan", out[k], mp.mpf(p["price"]), vc.cm_bar(case, p["e64"]), f"{name} payoff {k}"))
        if name == "tail":
            assert rec["tail"] < 1e-10 * model["S0"]
            assert abs(out[k] - float(mp.mpf(p["mixing"]))) <= 1e-10 * model["S0"], (k, out[k], p["mixing"])
    assert not [b for b in bad if b], bad
    one, alone = np.empty(1), [a[3:4].copy() for a in arrs]  # one workgroup per payoff: a payoff alone prices the same
    hhlib.check(hhlib.lib.hh_carr_madan_vg(hhlib.handle, C.byref(m), C.byref(g), rec["alpha"], rec["bound"],
                                           *[a.ctypes.data for a in alone], 1, one.ctypes.data))
    assert one[0] == out[3]


# ---- 10. errors ------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
BAD_VG = [  # (θ, ν, σ), text
    ((-0.3, 0.0, 0.2), "vg nu must be finite and > 0"), ((-0.3, -1.0, 0.2), "vg nu must be finite and > 0"),
    ((-0.3, NAN, 0.2), "vg nu must be finite and > 0"), ((-0.3, INF, 0.2), "vg nu must be finite and > 0"),
    ((NAN, 0.5, 0.2), "vg theta must be finite"), ((INF, 0.5, 0.2), "vg theta must be finite"),
    ((-INF, 0.5, 0.2), "vg theta must be finite"), ((-0.3, 0.5, -0.2), "sigma must be >= 0"),
    ((3.0, 0.5, 0.2), "1 - theta nu - sigma^2 nu / 2"), ((2.0, 0.5, 0.0), "1 - theta nu - sigma^2 nu / 2"),
    ((0.0, 0.5, 2.0), "1 - theta nu - sigma^2 nu / 2"),
]


def test_errors_come_back_without_a_launch(hhlib):
    """every HH_ERR_INVALID and HH_ERR_UNSUPPORTED case of the header through all four entry points, with its text; no timing
    slot is opened (nothing was launched); a good call afterwards returns what it returned before"""
    ctx = hhlib
    case = dict(vc.BASE)
    m, good = vc.model_of(case), vc.vg_of(case)
    n, steps = 300, 4
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    out, outs = _ffi.hh_result(), (_ffi.hh_result * 1)()
    pay = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.VANILLA, 100.0, 1.0))
    stats_buf = np.empty((_ffi.HH_PATH_STATS, n))
    exact = lambda **kw: terminal_config(n, 0, **kw)  # noqa: E731
    paths = lambda **kw: path_config(n, steps, 0, seeds, **kw)  # noqa: E731

    def term(mm, gg, cc):
        return ctx.lib.hh_mc_solve_vg(ctx.handle, mm, gg, cc, C.byref(out), None)

    def stat(mm, gg, cc, every=1):
        return ctx.lib.hh_mc_path_stats_vg(ctx.handle, mm, gg, cc, every, 0, stats_buf.ctypes.data, 0, None)

    def path(mm, gg, cc, every=1, arr=pay, k=1):
        return ctx.lib.hh_mc_solve_path_vg(ctx.handle, mm, gg, cc, every, 0, arr, k, outs, None, None)

    def expect(rc, code, text):
        assert rc == code, (rc, code, text, ctx.lib.hh_last_error(ctx.handle))
        assert text in ctx.lib.hh_last_error(ctx.handle).decode(), (text, ctx.lib.hh_last_error(ctx.handle))

    before, t_before = solve_vg(ctx, m, good, exact())
    res_before, _, stats_before = solve_path_vg(ctx, m, good, paths(), 2, 1, [pc.payoff(pc.VANILLA, 100.0, 1.0)])
    arrs = [np.array([x]) for x in (105.0, 1.0, 1.0, 0.03, math.exp(-0.03))]
    price = np.empty(1)

    def cm(mm, gg, alpha=1.5, bound=32.0, k=1):
        return ctx.lib.hh_carr_madan_vg(ctx.handle, mm, gg, alpha, bound, *[a.ctypes.data for a in arrs], k, price.ctypes.data)
    assert cm(C.byref(m), C.byref(good)) == _ffi.HH_OK
    cm_before = price[0]

    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
        for (theta, nu, sigma), text in BAD_VG:
            bad, mm = _ffi.make_vg(theta, nu), vc.model_of(dict(case, sigma=sigma))
            expect(term(C.byref(mm), C.byref(bad), C.byref(exact())), INV, "hh_mc_solve_vg: " + text)
            expect(stat(C.byref(mm), C.byref(bad), C.byref(paths())), INV, "hh_mc_path_stats_vg: " + text)
            expect(path(C.byref(mm), C.byref(bad), C.byref(paths())), INV, "hh_mc_solve_path_vg: " + text)
            expect(cm(C.byref(mm), C.byref(bad)), INV, "hh_carr_madan_vg: " + text)
        # the (1 + α)-th moment the damped transform needs: θ = 1.5, ν = 0.5 has E S_T finite and the 2.5-th moment not
        expect(cm(C.byref(m), C.byref(_ffi.make_vg(1.5, 0.5))), INV, "(1 + alpha)-th moment")
        # NULL arguments
        expect(term(C.byref(m), None, C.byref(exact())), INV, "hh_mc_solve_vg: NULL argument")
        expect(term(None, C.byref(good), C.byref(exact())), INV, "hh_mc_solve_vg: NULL argument")
        expect(stat(C.byref(m), None, C.byref(paths())), INV, "hh_mc_path_stats_vg: NULL argument")
        expect(path(C.byref(m), None, C.byref(paths())), INV, "hh_mc_solve_path_vg: NULL argument")
        expect(path(C.byref(m), C.byref(good), None), INV, "hh_mc_solve_path_vg: NULL argument")
        expect(cm(C.byref(m), None), INV, "hh_carr_madan_vg: NULL argument")
        # what the sibling entry points reject
        expect(term(C.byref(vc.model_of(dict(case, S0=-1.0))), C.byref(good), C.byref(exact())), INV, "S0 must be > 0")
        expect(term(C.byref(vc.model_of(dict(case, sigma=NAN))), C.byref(good), C.byref(exact())), INV, "model scalars must be finite")
        expect(term(C.byref(m), C.byref(good), C.byref(_ffi.make_config(GBM, EXACT, 0, 1, seeds=SEED))), INV, "n_paths must be >= 1")
        expect(term(C.byref(m), C.byref(good), C.byref(_ffi.make_config(GBM, EXACT, n, 1))), INV, "GENERATE needs seeds")
        expect(path(C.byref(m), C.byref(good), C.byref(paths()), every=3), INV, "must be >= 1 and divide n_steps")
        expect(stat(C.byref(m), C.byref(good), C.byref(paths()), every=0), INV, "must be >= 1 and divide n_steps")
        expect(path(C.byref(m), C.byref(good), C.byref(paths()), k=0), INV, "payoffs")
        expect(path(C.byref(m), C.byref(good), C.byref(paths()), arr=(_ffi.hh_path_payoff * 1)(pc.payoff(8, 100.0, 1.0))), INV, "unknown kind 8")
        expect(path(C.byref(vc.model_of(dict(case, T=INF))), C.byref(good), C.byref(paths())), INV, "model scalars finite")
        expect(cm(C.byref(m), C.byref(good), alpha=0.0), INV, "hh_carr_madan_vg: bad scalars")
        expect(cm(C.byref(m), C.byref(good), alpha=1e-4, bound=32.0), INV, "bound/alpha must be <= 196608")
        expect(cm(C.byref(m), C.byref(good), k=0), INV, "1 .. 2^20 payoffs per call")
        # unsupported
        needs = "needs LognormalDynamics + the exact law (HH_EXACT_LAW)"
        expect(term(C.byref(m), C.byref(good), C.byref(_ffi.make_config(HEST, _ffi.HH_BROADIE_KAYA, n, 1, seeds=SEED))), UNS, "hh_mc_solve_vg " + needs)
        expect(term(C.byref(m), C.byref(good), C.byref(_ffi.make_config(GBM, EULER, n, steps, seeds=SEED))), UNS, "hh_mc_solve_vg " + needs)
        expect(term(C.byref(m), C.byref(good), C.byref(exact(noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(n)))), UNS, "GENERATE noise, no dual partials")
        expect(term(C.byref(m), C.byref(good), C.byref(exact(n_partials=1))), UNS, "GENERATE noise, no dual partials")
        for call, who in ((stat, "hh_mc_path_stats_vg "), (path, "hh_mc_solve_path_vg ")):
            expect(call(C.byref(m), C.byref(good), C.byref(_ffi.make_config(HEST, EXACT, n, steps, seeds=seeds))), UNS, who + needs)
            expect(call(C.byref(m), C.byref(good), C.byref(_ffi.make_config(HEST, EULER, n, steps, seeds=seeds))), UNS, who + needs)
            expect(call(C.byref(m), C.byref(good), C.byref(_ffi.make_config(GBM, EULER, n, steps, seeds=seeds))), UNS, who + needs)
            expect(call(C.byref(m), C.byref(good), C.byref(_ffi.make_config(GBM, _ffi.HH_QE, n, steps, seeds=seeds))), UNS, who + needs)
            expect(call(C.byref(m), C.byref(good), C.byref(paths(noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4)))), UNS, "GENERATE noise, no dual partials")
            expect(call(C.byref(m), C.byref(good), C.byref(paths(n_partials=2))), UNS, "GENERATE noise, no dual partials")
        assert ctx.read_timings() == []  # nothing was launched
        # the context solves, and returns what it returned before
        after, t_after = solve_vg(ctx, m, good, exact())
        assert same_result(before, after) and np.array_equal(t_before, t_after)
        res_after, _, stats_after = solve_path_vg(ctx, m, good, paths(), 2, 1, [pc.payoff(pc.VANILLA, 100.0, 1.0)])
        assert same_result(res_before[0], res_after[0]) and np.array_equal(stats_before, stats_after)
        assert len(ctx.read_timings()) == 3  # one slot for the terminal law, two for the path form
        assert cm(C.byref(m), C.byref(good)) == _ffi.HH_OK and price[0] == cm_before > 0.0
        assert term(C.byref(m), C.byref(_ffi.make_vg(1.5, 0.5)), C.byref(exact())) == _ffi.HH_OK  # E S_T is finite there
    finally:
        ctx.enable_timing(False)


# ---- 11. Python is the C-ABI -----------------------------------------------------------------------------------------------

def test_python_routes(hhlib):
    """hh.solve on each payoff type equals the C call's result; a basket shares one simulation; CarrMadan and the analytic
    integral agree; a FiniteDifference Greek along ν is its two solves"""
    ref, exp_ = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
    mkt = hh.VarianceGammaInputs(ref, 0.03, 100.0, 0.2, -0.3, 0.5)
    call = hh.VanillaOption(100.0, exp_, hh.European(), hh.Call(), hh.Spot())
    prob = hh.PricingProblem(call, mkt)
    T = hh.yearfrac(ref, exp_)
    case = dict(vc.BASE, T=T, discount=hh.df(mkt.rate, exp_), r_drift=hh.zero_rate(mkt.rate, exp_))
    exact_price = hh.solve(prob, hh.VarianceGammaAnalytic()).price
    cm = hh.CarrMadan(1.5, 400.0, hh.VarianceGammaDynamics())
    assert hh.solve(prob, cm).price == pytest.approx(exact_price, abs=1e-7)  # a = 2: the tail beyond 400 decays like v^-5
    n, steps = 2 ** 14, 12
    seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    for vr, anti in ((hh.NoVarianceReduction(), 0), (hh.Antithetic(), 1)):
        method = hh.MonteCarlo(hh.VarianceGammaDynamics(), hh.VarianceGammaExact(),
                               hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=vr))
        sol = hh.solve(prob, method)
        c = _ffi.make_config(GBM, EXACT, n, steps, antithetic=anti, seeds=seeds)
        res, term = solve_vg(hhlib, vc.model_of(case, 100.0, 1.0), vc.vg_of(case), c)
        assert sol.price == res.price and sol.std_error == res.std_error
        ens = np.concatenate(sol.ensemble) if anti else sol.ensemble
        assert np.array_equal(ens, term) and abs(sol.price - exact_price) <= 4 * sol.std_error
        typed = [hh.AsianOption(100.0, exp_, hh.Call(), monitoring=hh.Monitoring(1)),
                 hh.AsianOption(100.0, exp_, hh.Put(), averaging=hh.GeometricAverage(), monitoring=hh.Monitoring(1)),
                 hh.BarrierOption(100.0, 80.0, exp_, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(1)),
                 hh.DigitalOption(101.0, exp_, hh.Put()),
                 hh.LookbackOption(exp_, hh.Call(), monitoring=hh.Monitoring(1)),
                 hh.LookbackOption(exp_, hh.Call(), strike=100.0, monitoring=hh.Monitoring(1))]
        packed = [hmc.pack_path_payoff(p) for p in typed + [call]]
        cres, _, cstats = solve_path_vg(hhlib, vc.model_of(case), vc.vg_of(case), c, 1, 0, packed)
        basket = hh.solve(hh.BasketPricingProblem(typed + [call], mkt), method, ensemble=True)
        for k, p in enumerate(typed):
            single = hh.solve(hh.PricingProblem(p, mkt), method)
            assert single.price == cres[k].price == basket.solutions[k].price and single.std_error == cres[k].std_error, k
            if not isinstance(p, hh.DigitalOption):  # (alone it is monitored at expiry only: other rows, the same S_T)
                assert np.array_equal(single.ensemble, cstats)
        assert basket.solutions[-1].price == cres[-1].price  # the vanilla rode along on the group's simulation
    fd = hh.FiniteDifference(1e-2)
    lens = hh.optic("market_inputs.nu")
    got = hh.solve(hh.GreekProblem(prob, lens), fd, method).greek
    up = hh.solve(hh.set(prob, lens, 0.5 * 1.01), method).price
    down = hh.solve(hh.set(prob, lens, 0.5 * 0.99), method).price
    assert got == (up - down) / (2 * 1e-2 * 0.5)
    want = hh.solve(hh.GreekProblem(prob, lens), fd, hh.VarianceGammaAnalytic()).greek
    assert got == pytest.approx(want, rel=0.25)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.ForwardAD(), method)
