"""State rows of the several-asset walk and the several-variable LSM on them (hh_assets.hip: assets_rows_kernel;
hh_lsm_multi.hip), against the statistics kernel, exact least squares, the one-variable induction and trees.  The numpy /
mpmath restatements and the derivation of every bar: tests/assets_lsm_cases.py.

Rows against the statistics kernel.  index_of restated on the returned rows must give hh_mc_path_stats_assets' rows.  The
index's x is exact in numpy (fma in rational arithmetic), so for the geometric, best-of and worst-of kinds the row SUM_X
— Σ x over the dates, in date order — is held to ==, on every divisor of 12.  The rows S_T, MAX_S, MIN_S and SUM_S of every
kind pass through the device's exp, which no test file restates: they are held to the bar assets_cases holds that
kernel's exp to (20·ε·|term|·max(|x|, 1) per exponential).
"""
import ctypes as C
import math

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from tests import assets_cases as ac
from tests import assets_lsm_cases as A

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ROWS, STEPS = 513, 12
DIVISORS = (1, 2, 3, 4, 6, 12)


@pytest.fixture(scope="module")
def ctx():
    return _ffi.Context(0)


def seeds_for(n):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(13)


def config(n, steps, anti=0, seeds=None):
    return _ffi.make_config(ac.GBM, ac.EULER, n, steps, antithetic=anti, seeds=seeds_for(n) if seeds is None else seeds)


def path_rows(ctx, case, kind, n, steps, every, anti):
    d = len(case["spots"])
    rows = np.full((steps // every + 1, d, n * (2 if anti else 1)), np.nan)
    assert rows.size == ctx.lib.hh_assets_rows_elems(n, steps // every, d, anti)
    m, a, c = ac.model_of(case), ac.assets_of(case, kind), config(n, steps, anti)
    ctx.check(ctx.lib.hh_assets_path_rows(ctx.handle, C.byref(m), C.byref(a), C.byref(c), every, rows.ctypes.data, 0, None))
    return rows


def path_stats(ctx, case, kind, n, steps, every, anti):
    stats = np.full((_ffi.HH_PATH_STATS, n * (2 if anti else 1)), np.nan)
    m, a, c = ac.model_of(case), ac.assets_of(case, kind), config(n, steps, anti)
    ctx.check(ctx.lib.hh_mc_path_stats_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), every, 0, stats.ctypes.data, 0,
                                              None))
    return stats


# ---- rows against the statistics kernel ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rows_cache(ctx):
    cache = {}

    def get(d, kind, anti, every=1, n=N_ROWS):
        extreme = kind in (ac.BEST, ac.WORST)   # the rows depend on the kind through x0 alone
        key = (d, extreme, anti, every, n)
        if key not in cache:
            cache[key] = path_rows(ctx, ac.path_case(d), kind, n, STEPS, every, anti)
        return cache[key]
    return get


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_rows_give_the_statistics_kernels_rows(ctx, rows_cache, d, anti):
    case = ac.path_case(d)
    w = case["weights"]
    for kind in ac.KINDS:
        full = rows_cache(d, kind, anti)
        if kind in (ac.SUM, ac.BEST):   # once per family of rows: date 0 is x0, and every divisor's rows are rows 0, m, 2m, …
            x0 = ac.constants_fp64(case, kind, STEPS, ac.cholesky_fp64(case["corr"]))[2]
            assert np.array_equal(full[0], np.repeat(np.array(x0)[:, None], full.shape[2], axis=1))
            for every in DIVISORS[1:]:
                assert np.array_equal(rows_cache(d, kind, anti, every), full[::every]), (kind, every)
        for every in DIVISORS:
            rows = full[::every]
            stats = path_stats(ctx, case, kind, N_ROWS, STEPS, every, anti)
            vals = [A.index_value(rows[j], w, kind) for j in range(1, rows.shape[0])]
            I, bar = np.array([t[0] for t in vals]), np.array([t[1] for t in vals])
            worst = 0.0
            for row, want, tol in ((_ffi.HH_STAT_S_T, I[-1], bar[-1]), (_ffi.HH_STAT_MAX_S, I.max(axis=0), bar.max(axis=0)),
                                   (_ffi.HH_STAT_MIN_S, I.min(axis=0), bar.max(axis=0)),
                                   (_ffi.HH_STAT_SUM_S, np.add.accumulate(I, axis=0)[-1], bar.sum(axis=0) + 2.0 ** -52 * len(I) * I.sum(axis=0))):
                err = np.abs(stats[row] - want)
                worst = max(worst, float(np.max(err / tol)))
                assert np.all(err <= tol), (kind, every, row, float(np.max(err / tol)))
            if kind != ac.SUM:
                xs = [A.index_log(rows[j], w, kind) for j in range(1, rows.shape[0])]
                assert np.array_equal(stats[_ffi.HH_STAT_SUM_X], np.add.accumulate(xs, axis=0)[-1]), (kind, every)
                if every == STEPS:     # one date: every S row is exp of the one x
                    for row in (_ffi.HH_STAT_MAX_S, _ffi.HH_STAT_MIN_S, _ffi.HH_STAT_SUM_S):
                        assert np.array_equal(stats[row], stats[_ffi.HH_STAT_S_T])
        print(f"\nd={d} anti={anti} kind={kind}: worst S-row error / bar {worst:.3f}")


@pytest.mark.parametrize("d", [2, 8])
def test_fewer_trajectories_are_the_same_columns_and_the_mirror_changes_none(ctx, rows_cache, d):
    plain, mirrored = rows_cache(d, ac.SUM, 0), rows_cache(d, ac.SUM, 1)
    assert np.array_equal(mirrored[:, :, :N_ROWS], plain)
    assert not np.array_equal(mirrored[1:, :, N_ROWS:], plain[1:])
    for n in (1, 63, 64, 65, 257):
        for anti in (0, 1):
            got = path_rows(ctx, ac.path_case(d), ac.SUM, n, STEPS, 3, anti)
            assert np.array_equal(got[:, :, :n], plain[::3, :, :n]), (n, anti)
            if anti:
                assert np.array_equal(got[:, :, n:], mirrored[::3, :, N_ROWS:N_ROWS + n]), n


# ---- sums and fits against exact least squares --------------------------------------------------------------------------

def states_desc(m, kind, cp, K, weights):
    d = _ffi.hh_lsm_states()
    d.kind, d.n_states, d.index_kind, d.cp, d.strike = _ffi.HH_LSM_STATES_LOG_ASSETS, m, kind, cp, K
    for i in range(m):
        d.weights[i] = weights[i]
    return d


def solve_states(ctx, rows, desc, degree, D, want_coef=True):
    n_dates, m, ntot = rows.shape[0] - 1, rows.shape[1], rows.shape[2]
    dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    B = len(A.basis(m, degree))
    tau, val, coef = np.zeros(ntot, dtype=np.int32), np.zeros(ntot), np.full((n_dates, B), np.nan)
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve_states(ctx.handle, C.byref(desc), dev.data_ptr(), ntot, n_dates, degree, D, C.byref(res),
                                          tau.ctypes.data, val.ctypes.data, coef.ctypes.data if want_coef else None))
    return res, tau, val, coef


def probe(ctx, x, xN, kind, weights, cp, K, D, degree):
    """One regression: the grid [x0, x, xN] -> (coef of date 1, exercised-at-date-1 mask, the exact fit, pay, itm)"""
    m, ntot = x.shape
    rows = np.stack([np.tile(np.log(100.0), (m, ntot)), x, xN])
    res, tau, val, coef = solve_states(ctx, rows, states_desc(m, kind, cp, K, weights), degree, D)
    assert np.all(coef[0] == 0.0)
    pay = cp * (A.index_value(x, weights, kind)[0] - K)
    itm = pay > 0.0
    assert np.all(tau[~itm] == 2)
    payN = np.maximum(cp * (A.index_value(xN, weights, kind)[0] - K), 0.0)
    y = math.exp(math.log(D)) * payN[itm]
    fit = A.exact_fit(np.exp(x), itm, y, A.basis(m, degree), ntot)
    assert (res.rows_regressed, res.rows_skipped) == ((1, 0) if itm.any() else (0, 1))
    return coef[1], tau == 1, fit, pay, itm


def check_probe(coef, exercised, fit, pay, itm):
    assert np.all(np.isfinite(coef))
    if not itm.any():
        assert np.all(coef == 0.0) and not exercised.any()
        return 0, 0
    dropped = [j for j in range(len(coef)) if j not in fit.kept]
    if not fit.ambiguous:
        assert np.all(coef[dropped] == 0.0), dropped
        err = np.abs(coef - fit.coef)
        assert np.all(err <= fit.dcoef), float(np.max(err[fit.kept] / fit.dcoef[fit.kept]))
    near = np.abs(pay[itm] - fit.fitted) <= fit.delta + 4 * A.U * np.abs(pay[itm])
    bad = (exercised[itm] != (pay[itm] > fit.fitted)) & ~near
    assert not bad.any(), int(bad.sum())
    return int(near.sum()), int(itm.sum())


def market(rng, m, ntot, spread=0.25):
    x = math.log(100.0) + spread * rng.standard_normal((m, ntot))
    return x, x + 0.1 * rng.standard_normal((m, ntot))


SHAPES = [(1, 3), (2, 1), (2, 3), (3, 2), (8, 2)]


@pytest.mark.parametrize("ntot", [1, 65, 513])
@pytest.mark.parametrize("m,p", SHAPES, ids=lambda v: str(v))
def test_one_regression_against_exact_least_squares(ctx, m, p, ntot):
    rng = np.random.default_rng(1000 * m + 10 * p + ntot)
    w = [1.0 / m] * m
    lines = []
    for kind, cp, K in ((ac.WORST, -1.0, 100.0), (ac.SUM, -1.0, 104.0), (ac.GEO, 1.0, 97.0)):
        wk = [1.0] * m if kind == ac.WORST else w
        x, xN = market(rng, m, ntot)
        coef, ex, fit, pay, itm = probe(ctx, x, xN, kind, wk, cp, K, 0.97, p)
        near, n_itm = check_probe(coef, ex, fit, pay, itm)
        assert fit.ambiguous or near <= 0.01 * n_itm + 2
        lines.append(f"kind {kind}: {n_itm} in the money, kept {len(fit.kept)} of {len(coef)}, {near} inside δ, cond {fit.cond:.1e}"
                     f"{' (ambiguous)' if fit.ambiguous else ''}")
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("m,p", [(2, 3), (8, 2)], ids=lambda v: str(v))
def test_hand_made_dates(ctx, m, p):
    rng = np.random.default_rng(m + p)
    B, ntot, K = len(A.basis(m, p)), 513, 100.0
    ones = [1.0] * m
    # fewer in-the-money columns than basis functions: pivots are dropped, their coefficients are 0
    x, xN = market(rng, m, ntot, 0.02)
    x += 0.3                                   # far out of the money for a worst-of put …
    x[:, :B - 3] -= 0.45                       # … except B − 3 columns
    coef, ex, fit, pay, itm = probe(ctx, x, xN, ac.WORST, ones, -1.0, K, 0.98, p)
    assert itm.sum() == B - 3
    check_probe(coef, ex, fit, pay, itm)
    assert np.sum(coef != 0.0) <= B - 3
    # none in the money: no fit, zeros
    coef, ex, fit, pay, itm = probe(ctx, x + 1.0, xN, ac.WORST, ones, -1.0, K, 0.98, p)
    check_probe(coef, ex, fit, pay, itm)
    # a constant regressor (v = exp(0) = 1 in every column: its sums are exact): the variance is not > 0, isd = 1, z = 0 —
    # every monomial in it is a dropped pivot
    x, xN = market(rng, m, ntot)
    x[0] = 0.0
    coef, ex, fit, pay, itm = probe(ctx, x, xN, ac.WORST, ones, -1.0, K, 0.98, p)
    check_probe(coef, ex, fit, pay, itm)
    with_z0 = [j for j, t in enumerate(A.basis(m, p)) if t[0] > 0]
    assert np.all(coef[with_z0] == 0.0)
    # two identical assets: a singular Gram matrix, no NaN
    x, xN = market(rng, m, ntot)
    x[1], xN[1] = x[0], xN[0]
    coef, ex, fit, pay, itm = probe(ctx, x, xN, ac.WORST, ones, -1.0, K, 0.98, p)
    check_probe(coef, ex, fit, pay, itm)


# ---- m = 1 against the one-variable induction, run to run -----------------------------------------------------------------

def gbm_rows(ctx, n, steps, every, kind=ac.WORST, anti=0):
    case = dict(spots=[100.0, 100.0], sigmas=[0.2, 0.3], weights=[1.0, 1.0] if kind in (ac.BEST, ac.WORST) else [0.5, 0.5],
                corr=[[1.0, 0.3], [0.3, 1.0]], r_drift=0.05, T=1.0)
    return case, path_rows(ctx, case, kind, n, steps, every, anti)


def test_one_state_row_is_the_one_variable_induction(ctx):
    n, steps, K, cp, degree = 4096, 8, 100.0, -1.0, 3
    case = dict(spots=[100.0], sigmas=[0.3], weights=[1.0], corr=[[1.0]], r_drift=0.05, T=1.0)
    rows = path_rows(ctx, case, ac.GEO, n, steps, 1, 0)
    D = math.exp(-0.05 / steps)
    res, tau, val, _ = solve_states(ctx, rows, states_desc(1, ac.GEO, cp, K, [1.0]), degree, D, want_coef=False)
    spots = np.ascontiguousarray(np.exp(rows[:, 0, :]))
    dev = torch.from_numpy(spots).cuda()
    torch.cuda.synchronize()
    m1 = _ffi.make_model(S0=100.0, sigma=0.3, r=0.05, T=1.0, strike=K, cp=cp)
    tau1, val1, res1 = np.zeros(n, dtype=np.int32), np.zeros(n), _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve_grid(ctx.handle, C.byref(m1), dev.data_ptr(), n, steps, degree, D, C.byref(res1),
                                        tau1.ctypes.data, val1.ctypes.data))
    # near-ties of the numpy restatement: |pay − cont| <= δ_t = 100·u·cond(G_t)·max|y| — a hundred times the first-order
    # size of a coefficient error of either induction on a Gram matrix of that condition number
    _, _, dates = A.numpy_lsm(rows, [1.0], ac.GEO, cp, K, degree, D)
    tie = np.zeros(n, dtype=bool)
    for t, (pay, cont, itm, cond, ymax) in dates.items():
        idx = np.nonzero(itm)[0]
        tie[idx[np.abs(pay - cont) <= 100 * A.U * cond * ymax]] = True
    assert tie.sum() <= 0.01 * n
    differ = tau != tau1
    assert not np.any(differ & ~tie), int(np.sum(differ & ~tie))
    d, d1 = D ** tau * val, D ** tau1 * val1
    assert abs(res.price - res1.price) <= float(np.sum(np.abs(d - d1)[tie])) / n + 1e-13 * res1.price
    print(f"\nm = 1: {int(differ.sum())} stopping times differ, {int(tie.sum())} near-ties; prices {res.price:.12f} / {res1.price:.12f}")


def test_the_same_call_twice_gives_the_same_bits(ctx):
    _, rows = gbm_rows(ctx, 5000, 8, 1)
    desc = states_desc(2, ac.WORST, -1.0, 100.0, [1.0, 1.0])
    a = solve_states(ctx, rows, desc, 3, 0.99)
    b = solve_states(ctx, rows, desc, 3, 0.99)
    assert a[0].price == b[0].price and a[0].std_error == b[0].std_error
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v)
    assert np.all(np.isfinite(a[3])) and np.any(a[3][1:] != 0.0)


# ---- prices -------------------------------------------------------------------------------------------------------------

PRICE_N, PRICE_STEPS, R, T, K = 1 << 17, 16, 0.05, 1.0, 100.0
TWO = dict(spots=[100.0, 100.0], sigmas=[0.2, 0.3], corr=[[1.0, 0.3], [0.3, 1.0]], r_drift=R, T=T)


def solve_assets(ctx, case, kind, weights, cp, every, degree=3, n=PRICE_N, steps=PRICE_STEPS):
    full = dict(case, weights=weights)
    m = _ffi.make_model(S0=1.0, V0=0.0, kappa=0.0, theta=0.0, sigma=0.0, rho=0.0, r=R, T=T, strike=K, cp=cp)
    a, c = ac.assets_of(full, kind), config(n, steps)
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), every, degree,
                                          math.exp(-R * T * every / steps), C.byref(res), None, None, None))
    return res, (m, a, c)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_one_exercise_date_is_the_european_price(ctx, kind):
    w = [1.0, 1.0] if kind in (ac.BEST, ac.WORST) else [0.5, 0.5]
    res, (m, a, c) = solve_assets(ctx, TWO, kind, w, -1.0, PRICE_STEPS)
    pay = _ffi.hh_path_payoff()
    pay.kind, pay.strike, pay.cp = _ffi.HH_PAYOFF_VANILLA, K, -1.0
    eu = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_solve_path_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), PRICE_STEPS, 0, C.byref(pay), 1,
                                              C.byref(eu), None, None))
    assert (res.rows_regressed, res.rows_skipped) == (0, 0)
    assert res.price == pytest.approx(eu.price, rel=1e-12)


def within_tree_bar(res, tree):
    return abs(res.price - tree) <= 0.02 * tree + 3 * res.std_error


def test_worst_of_and_basket_puts_against_the_two_asset_tree(ctx):
    for kind, w, payoff in ((ac.WORST, [1.0, 1.0], lambda a, b: np.maximum(K - np.minimum(a, b), 0.0)),
                            (ac.SUM, [0.5, 0.5], lambda a, b: np.maximum(K - 0.5 * (a + b), 0.0))):
        tree = A.beg_tree_put(TWO["spots"], TWO["sigmas"], 0.3, R, T, K, 128, PRICE_STEPS, payoff)
        am, _ = solve_assets(ctx, TWO, kind, w, -1.0, 1)
        eu, _ = solve_assets(ctx, TWO, kind, w, -1.0, PRICE_STEPS)
        four, _ = solve_assets(ctx, TWO, kind, w, -1.0, 4)
        print(f"\nkind {kind}: LSM {am.price:.4f} ± {am.std_error:.4f}, tree {tree:.4f}, European {eu.price:.4f}, 4 dates {four.price:.4f}")
        assert within_tree_bar(am, tree), (am.price, tree)
        assert am.price >= eu.price - 3 * am.std_error
        assert am.price >= four.price - 3 * am.std_error


def test_geometric_index_put_against_the_one_dimensional_tree(ctx):
    case = dict(spots=[100.0, 95.0, 105.0], sigmas=[0.2, 0.3, 0.25], corr=[[1.0, 0.3, 0.2], [0.3, 1.0, 0.4], [0.2, 0.4, 1.0]],
                r_drift=R, T=T)
    w = [1.0 / 3] * 3
    I0, vol, q = A.geometric_index_law(case["spots"], case["sigmas"], w, case["corr"])
    tree = A.crr_put_with_yield(I0, vol, R, q, T, K, 512, PRICE_STEPS)
    am, _ = solve_assets(ctx, case, ac.GEO, w, -1.0, 1)
    print(f"\ngeometric index of 3: LSM {am.price:.4f} ± {am.std_error:.4f}, tree {tree:.4f}")
    assert within_tree_bar(am, tree), (am.price, tree)


def test_print_the_index_only_price_beside_the_several_variable_price(ctx):
    n = 1 << 15
    case, rows = gbm_rows(ctx, n, PRICE_STEPS, 1)
    D = math.exp(-R * T / PRICE_STEPS)
    res, *_ = solve_states(ctx, rows, states_desc(2, ac.WORST, -1.0, K, [1.0, 1.0]), 3, D, want_coef=False)
    index = np.ascontiguousarray(np.exp(np.minimum(rows[:, 0], rows[:, 1])))
    dev = torch.from_numpy(index).cuda()
    torch.cuda.synchronize()
    m1 = _ffi.make_model(S0=100.0, sigma=0.3, r=R, T=T, strike=K, cp=-1.0)
    one = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve_grid(ctx.handle, C.byref(m1), dev.data_ptr(), n, PRICE_STEPS, 3, D, C.byref(one), None, None))
    print(f"\nworst-of put, {n} trajectories: two variables {res.price:.4f} ± {res.std_error:.4f}, the index alone {one.price:.4f}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_come_back_with_their_code_and_no_timing_slot(ctx):
    lib, h = ctx.lib, ctx.handle
    case = dict(TWO, weights=[1.0, 1.0])
    m = _ffi.make_model(S0=1.0, V0=0.0, kappa=0.0, theta=0.0, sigma=0.0, rho=0.0, r=R, T=T, strike=K, cp=-1.0)
    a, c = ac.assets_of(case, ac.WORST), config(64, 12)
    rows = np.zeros(lib.hh_assets_rows_elems(64, 12, 2, 0))
    res = _ffi.hh_lsm_result()
    dev = torch.zeros(3 * 2 * 64, dtype=torch.float64, device="cuda")
    desc = states_desc(2, ac.WORST, -1.0, K, [1.0, 1.0])
    INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
    ctx.check(lib.hh_ctx_enable_timing(h, 1))

    def edit(obj, **kw):
        out = type(obj).from_buffer_copy(obj)
        for k, v in kw.items():
            setattr(out, k, v)
        if hasattr(obj, "_keep"):
            out._keep = obj._keep
        return out

    def rows_call(m_=m, a_=a, c_=c, every=3, out=rows.ctypes.data):
        return lib.hh_assets_path_rows(h, C.byref(m_) if m_ else None, C.byref(a_) if a_ else None, C.byref(c_) if c_ else None,
                                       every, out, 0, None)

    def assets_call(m_=m, a_=a, c_=c, every=3, degree=3, D=0.99, out=res):
        return lib.hh_lsm_solve_assets(h, C.byref(m_) if m_ else None, C.byref(a_) if a_ else None, C.byref(c_) if c_ else None,
                                       every, degree, D, C.byref(out) if out else None, None, None, None)

    def states_call(d_=desc, ptr=dev.data_ptr(), ntot=64, n_dates=2, degree=3, D=0.99, out=res):
        return lib.hh_lsm_solve_states(h, C.byref(d_) if d_ else None, ptr, ntot, n_dates, degree, D, C.byref(out) if out else None,
                                       None, None, None)

    wide = ac.assets_of(ac.path_case(8), ac.SUM)
    cases = [
        (rows_call(m_=None), INV, "NULL argument"), (rows_call(a_=None), INV, "NULL argument"),
        (rows_call(out=None), INV, "NULL argument"), (rows_call(every=0), INV, "exercise_every"),
        (rows_call(every=5), INV, "exercise_every"), (rows_call(a_=edit(a, n_assets=9)), INV, "n_assets"),
        (rows_call(a_=edit(a, index_kind=7)), INV, "index_kind"), (rows_call(c_=edit(c, dynamics=_ffi.HH_HESTON)), UNS, "needs"),
        (rows_call(c_=edit(c, n_partials=1)), UNS, "GENERATE"), (rows_call(m_=edit(m, T=0.0)), INV, "T > 0"),
        (assets_call(out=None), INV, "NULL argument"), (assets_call(every=7), INV, "exercise_every"),
        (assets_call(degree=0), INV, "degree"), (assets_call(degree=9), INV, "degree"), (assets_call(D=0.0), INV, "LSM"),
        (assets_call(m_=edit(m, cp=0.5)), INV, "LSM"), (assets_call(a_=wide, degree=3), UNS, "basis functions"),
        (assets_call(c_=edit(c, strategy=_ffi.HH_EXACT_LAW)), UNS, "needs"), (assets_call(a_=edit(a, index_kind=-1)), INV, "index_kind"),
        (states_call(d_=None), INV, "NULL argument"), (states_call(ptr=None), INV, "NULL argument"),
        (states_call(out=None), INV, "NULL argument"), (states_call(ntot=0), INV, "LSM"), (states_call(n_dates=0), INV, "LSM"),
        (states_call(degree=9), INV, "degree"), (states_call(D=float("nan")), INV, "LSM"),
        (states_call(d_=edit(desc, kind=3)), INV, "descriptor kind"), (states_call(d_=edit(desc, n_states=0)), INV, "n_states"),
        (states_call(d_=edit(desc, n_states=9)), INV, "n_states"), (states_call(d_=edit(desc, index_kind=4)), INV, "index_kind"),
        (states_call(d_=edit(desc, cp=2.0)), INV, "LSM"), (states_call(d_=edit(desc, strike=float("inf"))), INV, "strike"),
        (states_call(d_=edit(desc, n_states=4), degree=4), UNS, "basis functions"),
        (states_call(d_=edit(desc, n_states=8), degree=3), UNS, "basis functions"),
    ]
    for k, (rc, code, words) in enumerate(cases):
        assert rc == code, (k, rc, code)
    # the message of the last one names the entry point and the count
    assert "hh_lsm_solve_states" in lib.hh_last_error(h).decode() and "basis functions" in lib.hh_last_error(h).decode()
    ms, n_out = (C.c_double * 8)(), C.c_int32(-1)
    ctx.check(lib.hh_ctx_read_timings(h, ms, 8, C.byref(n_out)))
    assert n_out.value == 0
    assert rows_call() == 0 and assets_call() == 0
    ctx.check(lib.hh_ctx_read_timings(h, ms, 8, C.byref(n_out)))
    assert n_out.value == 2
    ctx.check(lib.hh_ctx_enable_timing(h, 0))
