"""Several correlated lognormal assets on the device (hh_assets.hip) — hh_mc_path_stats_assets, hh_mc_solve_path_assets
and the Python routes above them.

  * PATH BY PATH against the restatement of tests/assets_cases.py at 50 digits, on the draws the device makes itself: the
    normals of domain 6 are restated from the oracle's host Philox words by hh_rng.h's formulas.  All five rows of both
    members within euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A); then every payoff kind on the device's own
    statistics against the numpy payoff table.
  * IDENTITIES, bit for bit: the antithetic call's first columns are the plain call's; a call is its two halves; an asset
    of weight zero and correlation zero changes nothing; at d = 1 the four index kinds agree; without volatility every
    date carries the index at the spots; a payoff's result does not depend on its neighbours.
  * THE LAW, fixed seeds: prices within 4 standard errors of closed forms that depend on the whole correlation matrix,
    which lie at least 69 standard errors from the same closed forms at zero correlation.
  * Errors: every HH_ERR_INVALID / HH_ERR_UNSUPPORTED case of the header, with its text, without a launch.
  * The Python routes end to end: the basket of examples/basket_rainbow.py.
The module prints its worst error/bar per kind of comparison at its end (`-s`)."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import assets_cases as ac  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import path_bridge_cases as bc  # noqa: E402
from tests import path_payoff_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = ac.load_golden()
MONITORED = _ffi.HH_EXTREMES_MONITORED
N = ac.PATH_N
_cache = {}


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("assets (device)")
    yield w
    w.report()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- calls ---------------------------------------------------------------------------------------------------------------

def config(n, n_steps, anti=0, seeds=None, **kw):
    seeds = ac.path_seeds()[:n] if seeds is None else seeds
    return _ffi.make_config(ac.GBM, ac.EULER, n, n_steps, antithetic=anti, seeds=seeds, **kw)


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def path_stats(ctx, case, kind, c, every, start):
    m, a = ac.model_of(case), ac.assets_of(case, kind)
    stats = np.empty((_ffi.HH_PATH_STATS, n_total(c)))
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), every, start, stats.ctypes.data,
                                              0, C.byref(res)))
    assert res.n_paths_done == c.n_paths and res.kernel_ms > 0.0
    return stats


def solve_path(ctx, case, kind, c, every, start, payoffs, want=True):
    m, a = ac.model_of(case), ac.assets_of(case, kind)
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = (np.empty((K, n_total(c))), np.empty((_ffi.HH_PATH_STATS, n_total(c)))) if want else (None, None)
    ctx.check(ctx.lib.hh_mc_solve_path_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), every, start, arr, K, res,
                                              values.ctypes.data if want else None, stats.ctypes.data if want else None))
    return list(res), values, stats


def same_result(a, b):
    return (a.price, a.std_error, a.sum_payoff, a.sumsq_payoff, a.n_paths_done) == \
        (b.price, b.std_error, b.sum_payoff, b.sumsq_payoff, b.n_paths_done)


# ---- (a) path by path ------------------------------------------------------------------------------------------------------
# (d, (n_steps, monitor_every), include_start, antithetic) per index kind: every d, every shape, both starts and both
# members with every kind; d = 3 and d = 8 under antithetic
SHAPES = [(1, (1, 1), 1, 0), (2, (5, 1), 0, 1), (3, (6, 3), 1, 1), (8, (5, 1), 0, 1)]
ALT = [(1, (6, 3), 0, 1), (2, (1, 1), 1, 0), (3, (5, 1), 0, 1), (8, (6, 3), 1, 1)]
PATH_CASES = [(kind,) + s for kind in ac.KINDS for s in (SHAPES if kind in (ac.SUM, ac.BEST) else ALT)]


@pytest.mark.parametrize("kind,d,shape,include_start,anti", PATH_CASES,
                         ids=[f"kind{k}-d{d}-{s[0]}x{s[1]}-start{st}-anti{a}" for k, d, s, st, a in PATH_CASES])
def test_path_by_path(hhlib, oracle, worst, kind, d, shape, include_start, anti):
    """All five rows of 257 trajectories — two workgroups, the second with one live lane — and of their mirrors; then
    every payoff kind on the device's own statistics."""
    n_steps, every = shape
    case, seeds = ac.path_case(d), ac.path_seeds()
    z8 = cached(("z", n_steps), lambda: ac.asset_normals(oracle, seeds, n_steps))
    z = [[row[:d] for row in path] for path in z8]
    ref = ac.path_reference(case, kind, z, anti, every, include_start)
    bars = etc.path_bar(ref["e64"], ref["A"])
    c = config(N, n_steps, anti)
    payoffs = ac.payoff_list(case, kind)
    res, values, stats = solve_path(hhlib, case, kind, c, every, include_start, payoffs)
    assert np.array_equal(stats, path_stats(hhlib, case, kind, c, every, include_start))
    bad = []
    for mem in range(ref["members"]):
        for i in range(N):
            for row in range(5):
                bad.append(worst.check(f"row {row}", stats[row][mem * N + i], ref["want"][mem][i][row], bars[mem][i][row],
                                       f"kind {kind} d={d} {n_steps}x{every} start={include_start} member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])
    n_mon = pc.n_mon(n_steps, every, include_start)
    for k, q in enumerate(payoffs):
        want = bc.payoff_from_stats(stats, q, n_mon, MONITORED)
        if q.kind == pc.GEOM:  # numpy's exp against the device's
            np.testing.assert_allclose(values[k], want, rtol=1e-14, atol=1e-13)
        else:
            assert np.array_equal(values[k], want), k
        pair = (values[k][:N] + values[k][N:]) / 2 if anti else values[k]
        assert res[k].sum_payoff == pytest.approx(math.fsum(pair), rel=1e-13, abs=1e-12)
        assert res[k].n_paths_done == N


# ---- (b) identities, bit for bit -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ac.KINDS)
def test_members_and_halves(hhlib, kind):
    """columns 0 … n−1 of an antithetic call are the plain call's; [0, n) is [0, k) followed by [k, n) with the seeds
    sliced — at sizes that are no multiple of the workgroup"""
    n, k, n_steps, every = 1000, 333, 6, 2
    case = ac.path_case(3)
    seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)
    plain = path_stats(hhlib, case, kind, config(n, n_steps, 0, seeds), every, 1)
    both = path_stats(hhlib, case, kind, config(n, n_steps, 1, seeds), every, 1)
    assert np.array_equal(both[:, :n], plain) and not np.array_equal(both[:, n:], plain)
    a = path_stats(hhlib, case, kind, config(k, n_steps, 1, seeds[:k]), every, 1)
    b = path_stats(hhlib, case, kind, config(n - k, n_steps, 1, seeds[k:]), every, 1)
    assert np.array_equal(both[:, :n], np.concatenate([a[:, :k], b[:, :n - k]], axis=1))
    assert np.array_equal(both[:, n:], np.concatenate([a[:, k:], b[:, n - k:]], axis=1))


@pytest.mark.parametrize("anti", [0, 1])
def test_an_asset_without_weight_or_correlation_changes_nothing(hhlib, anti):
    """d = 2, ρ = 0, weights (1, 0) is d = 1, weight 1, row for row (the sum and the geometric mean: the extremes admit no
    zero weight); and at d = 1, weight 1, the four index kinds give identical MAX_S, MIN_S and S_T"""
    n, n_steps = 600, 5
    one = dict(spots=[100.0], sigmas=[0.3], weights=[1.0], corr=[[1.0]], r_drift=0.03, T=0.75)
    two = dict(spots=[100.0, 80.0], sigmas=[0.3, 0.4], weights=[1.0, 0.0], corr=[[1.0, 0.0], [0.0, 1.0]], r_drift=0.03, T=0.75)
    c = config(n, n_steps, anti, np.arange(5, n + 5, dtype=np.uint64))
    rows = {kind: path_stats(hhlib, one, kind, c, 1, 1) for kind in ac.KINDS}
    for kind in (ac.SUM, ac.GEO):
        assert np.array_equal(path_stats(hhlib, two, kind, c, 1, 1), rows[kind]), kind
    for kind in ac.KINDS[1:]:
        for row in (pc.MAX_S, pc.MIN_S, pc.S_T):
            assert np.array_equal(rows[kind][row], rows[ac.SUM][row]), (kind, row)
    assert np.array_equal(rows[ac.GEO], rows[ac.BEST]) and np.array_equal(rows[ac.GEO], rows[ac.WORST])
    assert len(np.unique(rows[ac.SUM][pc.S_T])) > n // 2  # and they are paths, not constants


@pytest.mark.parametrize("kind", ac.KINDS)
def test_without_volatility_every_date_is_the_index_at_the_spots(hhlib, kind):
    """σ_i = 0, r = 0, d = 3, three dates (6 steps, every third, no start — and two plus the start): every trajectory
    carries the same rows, MAX = MIN = S_T, SUM_S = n_mon·S_T (2·I and 2·I + I are the correctly rounded 3·I), and
    S_T is within 4 ulp of numpy's index at the spots"""
    case = dict(ac.path_case(3), sigmas=[0.0, 0.0, 0.0], r_drift=0.0)
    I0 = ac.index_numpy(case, kind)
    for n_steps, every, start in ((6, 2, 0), (6, 3, 1)):
        stats = path_stats(hhlib, case, kind, config(N, n_steps, 1), every, start)
        n_mon = pc.n_mon(n_steps, every, start)
        assert n_mon == 3
        for row in range(5):
            assert len(np.unique(stats[row])) == 1, row
        S_T = stats[pc.S_T][0]
        assert stats[pc.MAX_S][0] == S_T and stats[pc.MIN_S][0] == S_T and stats[pc.SUM_S][0] == 3.0 * S_T
        assert abs(S_T - I0) <= 4 * np.spacing(I0)
        assert stats[pc.SUM_X][0] == pytest.approx(3.0 * math.log(I0), rel=1e-14)


def test_a_payoffs_result_does_not_depend_on_its_neighbours(hhlib):
    case, kind = ac.path_case(3), ac.WORST
    c = config(5000, 6, 1, np.arange(7, 5007, dtype=np.uint64))
    payoffs = ac.payoff_list(case, kind)
    together, _, _ = solve_path(hhlib, case, kind, c, 2, 0, payoffs, want=False)
    for k, q in enumerate(payoffs):
        alone, _, _ = solve_path(hhlib, case, kind, c, 2, 0, [q], want=False)
        assert same_result(alone[0], together[k]), k


# ---- (c) the law ----------------------------------------------------------------------------------------------------------------

LAW_N = 2 ** 18
LAW = [  # (case, golden name, index kind, weights or None, payoff, (n_steps, every, start))
    ("a", "geometric_call_K100", ac.GEO, None, pc.payoff(pc.VANILLA, 100.0, 1.0), (4, 1, 0)),
    ("b", "margrabe", ac.SUM, [1.0, -1.0], pc.payoff(pc.VANILLA, 0.0, 1.0), (4, 1, 0)),
    ("b", "worst_of_call_K100", ac.WORST, None, pc.payoff(pc.VANILLA, 100.0, 1.0), (4, 1, 0)),
    ("b", "best_of_call_K100", ac.BEST, None, pc.payoff(pc.VANILLA, 100.0, 1.0), (4, 1, 0)),
    ("a", "geometric_asian_K100", ac.GEO, None, pc.payoff(pc.GEOM, 100.0, 1.0), ac.ASIAN_SHAPE),
    ("e", "geometric_call_K100", ac.GEO, None, pc.payoff(pc.VANILLA, 100.0, 1.0), (4, 1, 0)),
]


def law_seeds():
    return cached("law seeds", lambda: np.arange(1, LAW_N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3))


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("cid,name,kind,weights,payoff,shape", LAW, ids=[f"{c}-{n}" for c, n, *_ in LAW])
def test_prices_against_closed_forms(hhlib, cid, name, kind, weights, payoff, shape, anti):
    """2¹⁸ trajectories, fixed seeds.  The log-Euler step is exact in law, so each price is held to 4 standard errors of
    its closed form (an honest implementation misses one such comparison with probability below 1e-4).  The closed form at
    zero correlation lies at least 69 of these standard errors from the correlated one — so at least 65 from any price that
    passes: the test cannot pass on uncorrelated draws."""
    case = dict(ac.CASES[cid], discount=math.exp(-ac.CASES[cid]["r_drift"] * ac.CASES[cid]["T"]))
    if weights is not None:
        case["weights"] = weights
    n_steps, every, start = shape
    res, _, _ = solve_path(hhlib, case, kind, config(LAW_N, n_steps, anti, law_seeds()), every, start, [payoff], want=False)
    r, rec = res[0], DOC["prices"][cid][name]
    want, flat = float(rec["price"]), float(rec["rho0"])
    miss, away = abs(r.price - want) / r.std_error, abs(want - flat) / r.std_error
    print(f"\n{cid} {name} antithetic={anti}: price {r.price:.6f} +- {r.std_error:.6f}, closed form {want:.6f}: {miss:.2f} "
          f"standard errors; zero correlation {flat:.6f}: {away:.1f} standard errors")
    assert r.std_error > 0.0 and miss <= 4.0, (name, r.price, want, r.std_error)
    assert away >= 69.0, (name, r.price, flat, r.std_error)


# ---- (d) errors -------------------------------------------------------------------------------------------------------------------

def test_errors_come_back_without_a_launch(hhlib):
    """every HH_ERR_INVALID and HH_ERR_UNSUPPORTED case of the header with its text; no timing slot is opened (nothing was
    launched) and the context solves afterwards to the known price"""
    ctx, case = hhlib, dict(ac.CASE_A)
    INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
    van = [pc.payoff(pc.VANILLA, 100.0, 1.0)]
    seeds = np.arange(1, 1025, dtype=np.uint64)

    def call(case=case, kind=ac.GEO, payoffs=van, assets=None, cfg=None, every=1, model=None, stats_form=False, n_assets=None):
        a = assets if assets is not None else ac.assets_of(case, kind)
        if n_assets is not None:
            a.n_assets = n_assets
        m = model if model is not None else ac.model_of(case)
        c = cfg if cfg is not None else config(1024, 4, 0, seeds)
        if stats_form:
            out = np.empty((5, n_total(c)))
            return ctx.lib.hh_mc_path_stats_assets(ctx.handle, C.byref(m), C.byref(a) if a else None, C.byref(c), every, 0,
                                                   out.ctypes.data, 0, None)
        arr = (_ffi.hh_path_payoff * len(payoffs))(*payoffs)
        res = (_ffi.hh_result * len(payoffs))()
        return ctx.lib.hh_mc_solve_path_assets(ctx.handle, C.byref(m), C.byref(a) if a else None, C.byref(c), every, 0, arr,
                                               len(payoffs), res, None, None)

    def expect(rc, code, text):
        msg = ctx.lib.hh_last_error(ctx.handle).decode()
        assert rc == code and text in msg, (rc, code, text, msg)

    NAN, INF = float("nan"), float("inf")
    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        for stats_form, who in ((False, "hh_mc_solve_path_assets"), (True, "hh_mc_path_stats_assets")):
            expect(call(assets=False, stats_form=stats_form), INV, who + ": NULL argument")
            for n in (0, 9, 2 ** 31):
                expect(call(n_assets=n, stats_form=stats_form), INV, "n_assets")
            for k in (-1, 4):
                expect(call(kind=k, stats_form=stats_form), INV, "unknown index_kind")
            for bad in (0.0, -1.0, NAN, INF):
                expect(call(dict(case, spots=[100.0, bad, 110.0]), stats_form=stats_form), INV, "asset 1: the spot must be finite and > 0")
            for bad in (-0.1, NAN, INF):
                expect(call(dict(case, sigmas=[0.2, 0.35, bad]), stats_form=stats_form), INV, "asset 2: sigma must be finite and >= 0")
            expect(call(dict(case, corr=[[1.0, 0.6, -0.3], [0.6, 0.99, 0.2], [-0.3, 0.2, 1.0]]), stats_form=stats_form), INV, "diagonal must be 1")
            expect(call(dict(case, corr=[[1.0, 0.6, -0.3], [0.6, 1.0, 0.2], [-0.3, 0.25, 1.0]]), stats_form=stats_form), INV, "not symmetric")
            for bad in (1.5, NAN, -INF):
                expect(call(dict(case, corr=[[1.0, bad, -0.3], [bad, 1.0, 0.2], [-0.3, 0.2, 1.0]]), stats_form=stats_form), INV, "not finite or lies outside")
            for Cm in ([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]], [[1.0, 1.0, 0.2], [1.0, 1.0, 0.2], [0.2, 0.2, 1.0]]):
                expect(call(dict(case, corr=Cm), stats_form=stats_form), INV, "not positive definite")
            for bad in (NAN, INF):
                expect(call(dict(case, weights=[0.5, bad, 0.2]), stats_form=stats_form), INV, "asset 1: the weight must be finite")
            expect(call(dict(case, weights=[0.0, 0.0, 0.0]), kind=ac.SUM, stats_form=stats_form), INV, "every weight of the weighted sum is zero")
            for kind in (ac.BEST, ac.WORST):
                for bad in (0.0, -1.0):
                    expect(call(dict(case, weights=[1.0, 1.0, bad]), kind=kind, stats_form=stats_form), INV, "weight must be > 0")
            # the model: only T, r_drift and discount are read
            for kw in (dict(T=0.0), dict(T=NAN), dict(r_drift=INF), dict(discount=NAN)):
                expect(call(dict(case, **kw), stats_form=stats_form), INV, "T > 0, r_drift and discount finite")
            # everything hh_mc_solve_path rejects
            expect(call(every=3, stats_form=stats_form), INV, "must be >= 1 and divide n_steps")
            expect(call(cfg=config(0, 4, 0, seeds), stats_form=stats_form), INV, "n_paths")
            c = config(1024, 4, 0, seeds)
            c.seeds = None
            expect(call(cfg=c, stats_form=stats_form), INV, "GENERATE needs seeds")
            # unsupported configurations
            for kw in (dict(dynamics=_ffi.HH_HESTON), dict(strategy=_ffi.HH_EXACT_LAW), dict(strategy=_ffi.HH_QE)):
                c = config(1024, 4, 0, seeds)
                for k, v in kw.items():
                    setattr(c, k, v)
                expect(call(cfg=c, stats_form=stats_form), UNS, "needs LognormalDynamics + EulerMaruyama")
            c = config(1024, 4, 0, seeds)
            c.noise_mode = _ffi.HH_NOISE_REPLAY
            expect(call(cfg=c, stats_form=stats_form), UNS, "GENERATE noise, no dual partials")
            c = config(1024, 4, 0, seeds)
            c.n_partials = 1
            expect(call(cfg=c, stats_form=stats_form), UNS, "GENERATE noise, no dual partials")
        # payoffs
        expect(call(dict(case, weights=[1.0, -1.0, 0.0]), kind=ac.SUM, payoffs=[van[0], pc.payoff(pc.GEOM, 5.0, 1.0)]), INV,
               "payoff 1: a geometric Asian on a weighted sum with a negative weight")
        expect(call(payoffs=[pc.payoff(8, 100.0, 1.0)]), INV, "unknown kind 8")
        expect(call(payoffs=[pc.payoff(pc.VANILLA, 100.0, 0.5)]), INV, "cp must be +1 or -1")
        assert ctx.read_timings() == []
    finally:
        ctx.enable_timing(False)
    # a geometric Asian on a spread is refused, on a geometric index with a negative weight it is not
    assert call(dict(case, weights=[1.0, -1.0, 0.5]), kind=ac.GEO, payoffs=[pc.payoff(pc.GEOM, 5.0, 1.0)]) == _ffi.HH_OK
    # and the context still solves: the d = 3 geometric-index call, to the price the law test holds to its closed form
    full = dict(ac.CASE_A, discount=math.exp(-0.03))
    res, _, _ = solve_path(ctx, full, ac.GEO, config(LAW_N, 4, 0, law_seeds()), 1, 0, van, want=False)
    want = float(DOC["prices"]["a"]["geometric_call_K100"]["price"])
    assert abs(res[0].price - want) <= 4.0 * res[0].std_error


# ---- (e) the Python routes end to end ------------------------------------------------------------------------------------------------

def _example():
    spec = importlib.util.spec_from_file_location("basket_rainbow", os.path.join(ROOT, "examples", "basket_rainbow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_python_routes(hhlib):
    """the basket of examples/basket_rainbow.py at 2¹⁶ trajectories: every solution is its single solve bit for bit; the
    prices are ordered as the payoffs are; the geometric-index call is within 4 standard errors of MultiAssetAnalytic and
    its bumped delta to the first asset within 5 % of the closed form's own finite difference (tests/test_gpu_merton.py's
    bar for a bumped spot)"""
    ex = _example()
    n = 2 ** 16
    opts, mkt, method = ex.options(), ex.market(), ex.method(n)
    names, payoffs = list(opts), list(opts.values())
    out = hh.solve(hh.BasketPricingProblem(payoffs, mkt), method)
    assert len(out.solutions) == len(payoffs) == 6
    for name, o, sol in zip(names, payoffs, out.solutions):
        single = hh.solve(hh.PricingProblem(o, mkt), method)
        assert isinstance(single, hh.MonteCarloSolution) and single.ensemble.shape == (5, 2 * n), name
        assert (single.price, single.std_error) == (sol.price, sol.std_error), name
        assert sol.price > 0.0 and sol.std_error > 0.0
    price = dict(zip(names, (s.price for s in out.solutions)))
    assert price["up-and-out basket call, B = 125"] < price["basket call, K = 100"]
    assert price["Asian basket call (arithmetic, monthly)"] < price["basket call, K = 100"]
    assert price["geometric index call, K = 100"] < price["basket call, K = 100"]  # AM-GM, payoff by payoff
    geo, sol = payoffs[-1], out.solutions[-1]
    prob = hh.PricingProblem(geo, mkt)
    closed = hh.solve(prob, hh.MultiAssetAnalytic()).price
    assert abs(sol.price - closed) <= 4.0 * sol.std_error
    fd = hh.FiniteDifference(1e-2)
    want = hh.solve(hh.GreekProblem(prob, hh.AssetSpotLens(0)), fd, hh.MultiAssetAnalytic()).greek
    got = hh.solve(hh.GreekProblem(prob, hh.AssetSpotLens(0)), fd, method).greek
    assert got == pytest.approx(want, rel=0.05) and want > 0.0
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.GreekProblem(prob, hh.AssetSpotLens(0)), hh.ForwardAD(), method)
