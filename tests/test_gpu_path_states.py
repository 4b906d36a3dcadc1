"""State rows (log spot, variance) of the stochastic-volatility walks (hh_mc_path_states) and Longstaff–Schwartz on (S, V)
(hh_lsm_solve_path_states; HH_LSM_STATES_LOG_SPOT_VARIANCE of hh_lsm_solve_states).  Restatements: tests/path_states_cases.py.

ROWS, bit for bit: the Euler source against hh_euler_grid's log states and variance grid; every source's x rows added in date
order against HH_STAT_SUM_X of its statistics call, the last v row of QE and Bates against var_T; a coarser grid against the
rows of the finest; one wave against many; the non-mirrored half of an antithetic grid against the plain one.  The QE and
Bates rows against the 50-digit walks of qe_cases.py / bates_cases.py on those modules' own models, seeds, shapes and bars:
the walks expose the log spot after every step — every x row is held — and the variance at expiry — the last v row is.

ONE REGRESSION against exact least squares (assets_lsm_cases.exact_fit, its bars and its "decisions outside δ exact" rule) on
the new kind's regressors, a grid on which the variance alone decides, and PRICES: the paired gain of the (S, V) policy over
the spot-only one on the same trajectories, the European price from below, one exercise date, Bates at λ = 0, run to run,
and a numpy restatement of the induction on the returned rows."""
import ctypes as C
import math

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from tests import assets_lsm_cases as A
from tests import path_grid_cases as pg
from tests import path_states_cases as ps

pytestmark = pytest.mark.gpu

SOURCES = ps.state_sources()
IDS = [s.name for s in SOURCES]
BIG, STEPS = ps.BIG, ps.STEPS
_R1 = {}


def finest(ctx, src, anti):
    """the 13 dates of BIG trajectories at exercise_every = 1 — computed once per source and mirror, never changed"""
    key = (src.name, anti)
    if key not in _R1:
        r = ps.path_states(ctx, src, src.model(), src.config(BIG, STEPS, anti), 1)
        r.setflags(write=False)
        _R1[key] = r
    return _R1[key]


# ---- 1. the rows are the states of the walks --------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [12, 7])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("src", SOURCES[:2], ids=IDS[:2])
def test_the_euler_source_is_hh_euler_grids_log_states_and_variance_grid(hhlib, src, anti, steps):
    m, c = src.model(), src.config(BIG, steps, anti)
    x = np.full((steps + 1, pg.n_total(c)), np.nan)
    v = np.full_like(x, np.nan)
    hhlib.check(hhlib.lib.hh_euler_grid(hhlib.handle, C.byref(m), C.byref(c), _ffi.HH_PATH_LOG, x.ctypes.data, v.ctypes.data, 0, None))
    rows = ps.path_states(hhlib, src, m, c, 1)
    assert np.array_equal(rows[:, 1], v) and np.array_equal(rows[:, 0], x)
    assert np.all(rows[0, 0] == math.log(m.S0)) and np.all(rows[0, 1] == m.V0)


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("src", SOURCES, ids=IDS)
def test_rows_against_the_statistics_and_a_coarser_grid_against_the_finest(hhlib, src, anti):
    R1 = finest(hhlib, src, anti)
    m, c = src.model(), src.config(BIG, STEPS, anti)
    assert R1.shape == (STEPS + 1, 2, BIG * (1 + anti)) and np.all(np.isfinite(R1))
    assert np.all(R1[0, 0] == math.log(m.S0)) and np.all(R1[0, 1] == m.V0)
    for every in ps.DIVISORS:
        rows = R1 if every == 1 else ps.path_states(hhlib, src, m, c, every)
        assert rows.shape[0] == STEPS // every + 1 and np.array_equal(rows, R1[::every]), (src.name, every)
        stats, var_T = ps.stats_with_var_T(hhlib, src, m, c, every)
        total = rows[1, 0].copy()
        for j in range(2, rows.shape[0]):  # one rounded addition per date, in date order
            total = total + rows[j, 0]
        assert np.array_equal(stats[_ffi.HH_STAT_SUM_X], total), (src.name, every)
        if var_T is not None:
            assert np.array_equal(rows[-1, 1], var_T) and np.all(var_T >= 0.0), (src.name, every)


@pytest.mark.parametrize("src", SOURCES, ids=IDS)
def test_fewer_trajectories_are_the_same_columns_and_the_mirror_changes_none(hhlib, src):
    plain, mirrored = finest(hhlib, src, 0), finest(hhlib, src, 1)
    assert np.array_equal(mirrored[:, :, :BIG], plain)
    assert not np.array_equal(mirrored[1:, :, BIG:], plain[1:])
    seeds = pg.seeds_for(BIG, 17)
    for n in ps.SIZES:
        for anti in (0, 1):
            got = ps.path_states(hhlib, src, src.model(), src.config(n, STEPS, anti, seeds=seeds[:n]), 3)
            assert np.array_equal(got[:, :, :n], plain[::3, :, :n]), (src.name, n, anti)
            if anti:
                assert np.array_equal(got[:, :, n:], mirrored[::3, :, BIG:BIG + n]), (src.name, n)


# ---- 2. the QE and Bates rows against the 50-digit walks --------------------------------------------------------------------

def _states_against_the_walks(ctx, worst, family, name, case, src, config, runs_of, n_steps, every, anti, mart, reference):
    """x of date j at exercise_every = m is the log spot after step j·m: SUM_X of the restatement's rows over the first j·m
    steps monitored at j·m alone; v of the last date is the restatement's var_T (its row 5) — each at the module's own bar,
    euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A)."""
    from tests import euler_tangent_cases as etc
    m = src.model(T=case["T"])
    rows = ps.path_states(ctx, src, m, config(anti), every)
    n = rows.shape[2] // (1 + anti)
    assert np.all(rows[0, 0] == math.log(case["S0"])) and np.all(rows[0, 1] == case["V0"])
    runs = runs_of()[:1 + anti]
    bad = []
    n_dates = n_steps // every
    for j in range(1, n_dates + 1):
        upto = j * every
        cut = [[(xs_mp[:upto], v_mp, xs_64[:upto], v_64) for xs_mp, v_mp, xs_64, v_64 in member] for member in runs]
        ref = reference(case, cut, upto, 0)
        bars = etc.path_bar(ref["e64"], ref["A"])
        where = f"{name} {n_steps} steps every={every} anti={anti} mart={mart} date {j}"
        for mem in range(1 + anti):
            for i in range(n):
                bad.append(worst.check(f"{family} x row", rows[j, 0, mem * n + i], ref["want"][mem][i][_ffi.HH_STAT_SUM_X],
                                       bars[mem][i][_ffi.HH_STAT_SUM_X], f"{where} member {mem} path {i}"))
                if j == n_dates:  # the walk exposes the variance at expiry alone
                    bad.append(worst.check(f"{family} v row", rows[j, 1, mem * n + i], ref["want"][mem][i][5], bars[mem][i][5],
                                           f"{where} member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


@pytest.fixture(scope="module")
def worst_rows():
    from tests import euler_tangent_cases as etc
    w = etc.Worst("state rows (device)")
    yield w
    w.report()


@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1), (5, 1), (6, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["feller", "low_v0"])
def test_qe_states_against_the_50_digit_walk(hhlib, oracle, worst_rows, name, shape, anti, mart):
    """qe_cases' own models, seeds (257 trajectories) and shapes; the walks are test_gpu_qe.py's, computed once a session"""
    from tests import qe_cases as qc
    from tests import test_gpu_qe as tq
    assert shape in qc.PATH_SHAPES and name in qc.MODELS
    n_steps, every = shape
    case, seeds = qc.MODELS[name], qc.path_seeds()
    Z = tq.cached(("Z", n_steps), lambda: qc.step_normals(oracle, seeds, n_steps))
    U = tq.cached(("U", n_steps), lambda: qc.step_uniforms(oracle, seeds, n_steps))
    _states_against_the_walks(hhlib, worst_rows, "qe", name, case, pg.qe(mart, case, f"qe-{name}"),
                              lambda anti: qc.config_of(qc.PATH_N, n_steps, seeds, anti),
                              lambda: tq.cached(("runs", name, n_steps, mart), lambda: qc.walks(case, n_steps, Z, U, 1, mart)[0]),
                              n_steps, every, anti, mart, qc.reference)


@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1), (5, 1), (6, 1), (6, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["feller", "low_v0"])
def test_bates_states_against_the_50_digit_walk(hhlib, oracle, worst_rows, name, shape, anti, mart):
    """bates_cases' own models, jumps (λ·dt = 0.9), seeds and shapes; the walks are test_gpu_bates.py's"""
    from tests import bates_cases as bt
    from tests import test_gpu_bates as tb
    assert shape in bt.PATH_SHAPES and name in bt.MODELS
    n_steps, every = shape
    case, seeds = bt.path_case(name, n_steps), bt.path_seeds()
    d = tb.cached(("d", n_steps), lambda: bt.draws(oracle, seeds, n_steps))
    N = tb.cached(("N", name, n_steps), lambda: bt.counts(d["UJ"], bt.path_mean(case, n_steps)))
    _states_against_the_walks(hhlib, worst_rows, "bates", name, case, pg.bates(mart, lam=case["lam"], case=case, name=f"bates-{name}"),
                              lambda anti: bt.config_of(bt.PATH_N, n_steps, seeds, anti),
                              lambda: tb.cached(("runs", name, n_steps, mart), lambda: bt.walks(case, n_steps, d, N, 1, mart)[0]),
                              n_steps, every, anti, mart, bt.reference)


# ---- 3. one regression against exact least squares --------------------------------------------------------------------------

def probe(ctx, x, xN, cp, K, D, degree):
    """One regression: the grid [start, x, xN] of (log spot, variance) rows -> (coef of date 1, exercised-at-date-1 mask, the
    exact fit, pay, itm), as test_gpu_assets_lsm.probe"""
    from tests.test_gpu_assets_lsm import solve_states
    ntot = x.shape[1]
    rows = np.stack([np.stack([np.full(ntot, math.log(100.0)), np.full(ntot, 0.04)]), x, xN])
    res, tau, val, coef = solve_states(ctx, rows, ps.desc(cp, K), degree, D)
    assert np.all(coef[0] == 0.0)
    pay = ps.pay_of(x, cp, K)
    itm = pay > 0.0
    assert np.all(tau[~itm] == 2)
    y = math.exp(math.log(D)) * np.maximum(ps.pay_of(xN, cp, K), 0.0)[itm]
    fit = A.exact_fit(ps.regressors(x), itm, y, A.basis(2, degree), ntot)
    assert (res.rows_regressed, res.rows_skipped) == ((1, 0) if itm.any() else (0, 1))
    return coef[1], tau == 1, fit, pay, itm


def market(rng, ntot, spread=0.25):
    """log spots about log 100 and variances about 0.09 (some negative, as the Euler walk leaves them), then a later date"""
    x = np.stack([math.log(100.0) + spread * rng.standard_normal(ntot), 0.09 + 0.05 * rng.standard_normal(ntot)])
    return x, np.stack([x[0] + (0.1 + np.sqrt(np.abs(x[1]))) * 0.3 * rng.standard_normal(ntot), x[1]])


@pytest.mark.parametrize("ntot", [65, 513])
@pytest.mark.parametrize("degree", [1, 3, 8])
def test_one_regression_against_exact_least_squares(hhlib, degree, ntot):
    from tests.test_gpu_assets_lsm import check_probe
    rng = np.random.default_rng(100 * degree + ntot)
    lines = []
    for cp, K in ((-1.0, 100.0), (-1.0, 110.0), (1.0, 97.0)):
        x, xN = market(rng, ntot)
        coef, ex, fit, pay, itm = probe(hhlib, x, xN, cp, K, 0.97, degree)
        near, n_itm = check_probe(coef, ex, fit, pay, itm)
        # that δ is no empty bar is asked where the fit is well posed, B <= 10 functions on these columns (condition numbers
        # about 10 – 100).  The 45 monomials of degree 8 on a few dozen to a few hundred columns are close to an interpolation
        # (condition number 10^9 and more on 47 columns): there δ is wide by its derivation, and the count is printed
        assert degree == 8 or fit.ambiguous or near <= 0.01 * n_itm + 2
        lines.append(f"cp {cp:+.0f} K {K:g}: {n_itm} in the money, kept {len(fit.kept)} of {len(coef)}, {near} inside δ, "
                     f"cond {fit.cond:.1e}{' (ambiguous)' if fit.ambiguous else ''}")
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("degree", [1, 3, 8])
def test_hand_made_dates(hhlib, degree):
    from tests.test_gpu_assets_lsm import check_probe
    rng = np.random.default_rng(degree)
    B, ntot, K = len(A.basis(2, degree)), 513, 100.0
    # fewer in-the-money columns than basis functions (B − 1 >= 2 of them): pivots are dropped, their coefficients are 0
    x, xN = market(rng, ntot, 0.02)
    x[0] += 0.3                                # far out of the money for a put …
    x[0, :B - 1] -= 0.45                       # … except B − 1 columns
    coef, ex, fit, pay, itm = probe(hhlib, x, xN, -1.0, K, 0.98, degree)
    assert itm.sum() == B - 1
    check_probe(coef, ex, fit, pay, itm)
    assert np.sum(coef != 0.0) <= B - 1
    # none in the money: no fit, zeros
    x[0] += 1.0
    coef, ex, fit, pay, itm = probe(hhlib, x, xN, -1.0, K, 0.98, degree)
    check_probe(coef, ex, fit, pay, itm)
    # a variance row constant across the columns (σ = 0, κ = 0: every trajectory keeps V0 — here 2^-4, whose sums are exact):
    # the regressor's variance is not > 0, isd = 1, z_1 = 0 — every monomial in it is a dropped pivot
    x, xN = market(rng, ntot)
    x[1] = xN[1] = 0.0625
    coef, ex, fit, pay, itm = probe(hhlib, x, xN, -1.0, K, 0.98, degree)
    check_probe(coef, ex, fit, pay, itm)
    with_z1 = [j for j, t in enumerate(A.basis(2, degree)) if t[1] > 0]
    assert np.all(coef[with_z1] == 0.0) and np.any(coef != 0.0)


def test_a_constant_variance_row_from_the_walk_itself(hhlib):
    """σ = 0 and κ = 0 on the Euler source: the v rows are V0 in every column and on every date, and the solve drops every
    monomial in the variance"""
    src = pg.euler("euler-const-v", pg.HES, dict(pg.H252, V0=0.0625, kappa=0.0, sigma=0.0))
    m, c = src.model(strike=100.0, cp=-1.0), src.config(BIG, STEPS)
    res, tau, val, coef, rows = ps.lsm_states(hhlib, src, m, c, 3, 3, ps.date_discount(m, STEPS, 3), want_rows=True, want_coef=True)
    assert np.all(rows[:, 1] == 0.0625)
    with_z1 = [j for j, t in enumerate(A.basis(2, 3)) if t[1] > 0]
    assert np.all(coef[:, with_z1] == 0.0) and np.any(coef[1:] != 0.0) and np.all(np.isfinite(coef))
    assert res.rows_regressed == 3 and res.price > 0.0


# ---- 4. a grid on which the variance alone decides --------------------------------------------------------------------------

def test_the_variance_alone_decides(hhlib):
    from tests.test_gpu_assets_lsm import solve_states
    rows, v = ps.variance_decides_grid(513)
    n = v.size
    res, tau, val, coef = solve_states(hhlib, rows, ps.desc(-1.0, 100.0), 1, 1.0)
    pay1, pay2 = ps.pay_of(rows[1], -1.0, 100.0), ps.pay_of(rows[2], -1.0, 100.0)
    assert np.all(pay1 > 0.0) and np.all(pay2 > 0.0)
    fit = A.exact_fit(ps.regressors(rows[1]), pay1 > 0.0, pay2, A.basis(2, 1), n)
    # the spot is the same in every column: its monomial is a dropped pivot, the fit is 1 and z_1 alone
    assert coef[1][1] == 0.0 and coef[1][0] != 0.0 and coef[1][2] != 0.0
    assert np.max(np.abs(fit.fitted - (10.0 - 200.0 * (v - 0.04)))) < 1e-9
    near = np.abs(pay1 - fit.fitted) <= fit.delta + 4 * A.U * np.abs(pay1)
    left_out = near | (np.abs(v - 0.04) * 200.0 <= fit.delta)
    assert left_out.sum() <= 2, int(left_out.sum())
    exercised = tau == 1
    assert np.array_equal(exercised[~left_out], (v > 0.04)[~left_out])
    assert np.all(tau[~exercised] == 2)
    closed = float(np.sum(np.where(exercised, pay1, pay2))) / n   # D = 1: the undiscounted mean of what each column takes
    print(f"\n{int(exercised.sum())} of {n} exercise, {int(left_out.sum())} inside δ (max δ {float(np.max(fit.delta)):.2e}); "
          f"price {res.price!r}, closed sum {closed!r}")
    assert np.array_equal(exercised, v > 0.04)   # none is that close: the nearest column lies 0.02/513 from 0.04
    assert res.price == pytest.approx(closed, rel=1e-12)


# ---- 5. prices ---------------------------------------------------------------------------------------------------------------

_SOLVED = {}


def solved(ctx, which, name):
    """the (S, V) solve of a price case with its rows, once per session"""
    key = (which, name)
    if key not in _SOLVED:
        src = ps.price_source(which, name)
        m, c = ps.price_case(src, name)
        D = ps.date_discount(m, ps.PRICE_STEPS, ps.PRICE_EVERY)
        out = ps.lsm_states(ctx, src, m, c, ps.PRICE_EVERY, ps.DEGREE, D, want_rows=True)
        for a in out[1:]:
            if a is not None:
                a.setflags(write=False)
        _SOLVED[key] = (src, m, c, D) + out
    return _SOLVED[key]


@pytest.mark.parametrize("name", ["wild", "mid"])
@pytest.mark.parametrize("which", ["euler", "qe"])
def test_the_paired_gain_over_the_spot_only_policy(hhlib, which, name):
    """Both solves on the same seeds: per trajectory D^τ·val of the (S, V) policy less that of the spot-only policy
    (hh_lsm_solve_path on the source's spot rows); the mean of the differences is at least 10 of its standard errors."""
    src, m, c, D, sv, tau, val, _, _ = solved(hhlib, which, name)
    s_only, tau_s, val_s, _ = pg.lsm_path(hhlib, src, m, c, ps.PRICE_EVERY, ps.DEGREE, D, want_grid=False)
    diff = D ** tau * val - D ** tau_s * val_s
    gain, se = float(diff.mean()), float(diff.std(ddof=1) / math.sqrt(diff.size))
    print(f"\n{which} {name}: (S, V) {sv.price:.4f} ± {sv.std_error:.4f}, S alone {s_only.price:.4f}, paired gain {gain:.4f} = "
          f"{gain / se:.1f} standard errors")
    assert sv.price == pytest.approx(float(np.mean(D ** tau * val)), rel=1e-12)
    assert gain >= 10.0 * se, (gain, se)


@pytest.mark.parametrize("name", ["wild", "mid"])
@pytest.mark.parametrize("which", ["euler", "qe", "bates"])
def test_the_price_is_not_below_the_european(hhlib, which, name):
    src, m, c, D, sv, *_ = solved(hhlib, which, name)
    eu = src.vanilla(hhlib, m, c)
    print(f"\n{which} {name}: (S, V) {sv.price:.4f} ± {sv.std_error:.4f}, European {eu.price:.4f} ± {eu.std_error:.4f}")
    assert sv.price >= eu.price - 3 * math.hypot(sv.std_error, eu.std_error)


@pytest.mark.parametrize("which", ["euler", "qe", "bates"])
def test_one_exercise_date_is_the_european_solve(hhlib, which):
    src = ps.price_source(which, "mid")
    m, c = ps.price_case(src, "mid")
    res, *_ = ps.lsm_states(hhlib, src, m, c, ps.PRICE_STEPS, ps.DEGREE, m.discount)
    eu = src.vanilla(hhlib, m, c)
    assert (res.rows_regressed, res.rows_skipped) == (0, 0)
    assert res.price == pytest.approx(eu.price, rel=1e-12)


def test_bates_without_jumps_is_the_qe_solve_and_a_second_run_gives_the_same_bits(hhlib):
    _, m, c, D, res, tau, val, _, rows = solved(hhlib, "qe", "mid")
    b = pg.bates(1, 0.0, ps.HESTON["mid"], "bates-lam0")
    for src in (b, ps.price_source("qe", "mid")):
        again = ps.lsm_states(hhlib, src, b.model(T=m.T, strike=m.strike, cp=m.cp), c, ps.PRICE_EVERY, ps.DEGREE, D, want_rows=True)
        assert (again[0].price, again[0].std_error, again[0].rows_regressed) == (res.price, res.std_error, res.rows_regressed)
        assert np.array_equal(again[1], tau) and np.array_equal(again[2], val) and np.array_equal(again[4], rows)


@pytest.mark.parametrize("which,name", [("euler", "wild"), ("qe", "mid")])
def test_a_numpy_restatement_of_the_induction_on_the_returned_rows(hhlib, which, name):
    """test_gpu_assets_lsm's bar for its own price comparison: a decision may differ from the restatement's only on a near-tie,
    |pay − cont| <= 100·u·cond(G_t)·max|y| — a hundred times the first-order size of a coefficient error of either induction
    on a Gram matrix of that condition number; near-ties are at most 1 % of the columns; and the prices differ by no more
    than the near-ties' discounted values do, plus 1e-13 of the price."""
    src, m, c, D, res, tau, val, _, rows = solved(hhlib, which, name)
    n = tau.size
    assert np.array_equal(rows, ps.path_states(hhlib, src, m, c, ps.PRICE_EVERY))
    price, tau_np, val_np, dates = ps.numpy_lsm(rows, -1.0, ps.STRIKE, ps.DEGREE, D)
    tie = np.zeros(n, dtype=bool)
    for t, (pay, cont, itm, cond, ymax) in dates.items():
        idx = np.nonzero(itm)[0]
        tie[idx[np.abs(pay - cont) <= 100 * A.U * cond * ymax]] = True
    differ = tau != tau_np
    print(f"\n{which} {name}: device {res.price:.12f}, numpy {price:.12f}; {int(differ.sum())} stopping dates differ, "
          f"{int(tie.sum())} near-ties, worst cond {max(d[3] for d in dates.values()):.1e}")
    assert tie.sum() <= 0.01 * n
    assert not np.any(differ & ~tie), int(np.sum(differ & ~tie))
    d, d_np = D ** tau * val, D ** tau_np * val_np
    assert abs(res.price - price) <= float(np.sum(np.abs(d - d_np)[tie])) / n + 1e-13 * price


# ---- 6. the host mirror ------------------------------------------------------------------------------------------------------

def test_host_mirror(hhlib):
    import hedgehog_jl_amd as hh
    ref, exp = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
    n, steps, every = 20_000, 24, 4
    cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64))
    put = hh.VanillaOption(100.0, exp, hh.American(), hh.Put(), hh.Spot())
    mkt = hh.HestonInputs(ref, 0.05, 100.0, 0.09, 1.0, 0.09, 1.0, -0.3)
    prob = hh.PricingProblem(put, mkt)
    for method, kw in ((hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, 3), dict(path_state="spot")),
                       (hh.LSM(hh.HestonDynamics(), hh.HestonQE(), cfg, 3), {})):
        sv = hh.solve(prob, method, exercise_every=every, regressors="spot_variance", spot_paths=True, **kw)
        s = hh.solve(prob, method, exercise_every=every, spot_paths=True, **kw)
        assert isinstance(sv, hh.LSMSolution) and sv.spot_paths.shape == (steps // every + 1, n)
        paths = hh.simulate_state_paths(prob, method.mc_method, exercise_every=every)
        assert np.array_equal(paths.spot, sv.spot_paths) and paths.variance.shape == paths.spot.shape
        assert paths.times.size == steps // every + 1 and np.all(paths.variance[0] == 0.09)
        # exp of the stored log spot on the host, exp of the state on the device: the same number up to both roundings
        np.testing.assert_allclose(paths.spot, s.spot_paths, rtol=1e-14)
        tau, _ = sv.stopping_info
        assert tau.min() >= 1 and tau.max() <= steps // every
        assert sv.price > s.price - 3 * math.hypot(sv.std_error, s.std_error)


# ---- 7. refusals: all of them before any launch -----------------------------------------------------------------------------

def test_every_refusal_comes_back_before_a_launch(hhlib):
    ctx = hhlib
    n, steps = 300, 12
    INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
    rows = np.empty((steps + 1, 2, n))
    out = _ffi.hh_lsm_result()

    def both(source, m, c, every=1, degree=3, D=0.99):
        a = ctx.lib.hh_mc_path_states(ctx.handle, source, m, c, every, rows.ctypes.data, 0, None)
        ta = ctx.lib.hh_last_error(ctx.handle).decode()
        b = ctx.lib.hh_lsm_solve_path_states(ctx.handle, source, m, c, every, degree, D, C.byref(out), None, None, None, None)
        return (a, ta), (b, ctx.lib.hh_last_error(ctx.handle).decode())

    def expect(source, m, c, code, text, named=True, **kw):
        for who, (rc, msg) in zip(("hh_mc_path_states", "hh_lsm_solve_path_states"), both(source, m, c, **kw)):
            assert rc == code and text in msg and (who in msg or not named), (who, rc, code, text, msg)

    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        for src in SOURCES:
            s, m, c = src.source(), src.model(), src.config(n, steps)
            S, M, Cc = C.byref(s), C.byref(m), C.byref(c)
            expect(None, M, Cc, INV, "NULL argument")
            expect(S, None, Cc, INV, "NULL argument")
            expect(S, M, None, INV, "NULL argument")
            for field in src.structs:  # a struct the kind needs
                bare = _ffi.make_path_source(src.kind, **{k: v for k, v in src.structs.items() if k != field})
                expect(C.byref(bare), M, Cc, INV, "NULL argument")
            for every in (0, 5, 24):
                expect(S, M, Cc, INV, "exercise_every", every=every)
            expect(S, M, C.byref(src.config(n, 0)), INV, "n_steps", named=False)
            expect(S, M, C.byref(src.config(0, steps)), INV, "n_paths", named=False)
            expect(S, M, C.byref(src.config(n, steps, noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4))), UNS,
                   "GENERATE noise, no dual partials")
            expect(S, M, C.byref(src.config(n, steps, n_partials=2)), UNS, "GENERATE noise, no dual partials")
            for dyn, strat in ((pg.GBM, pg.EM), (pg.HES, pg.EM), (pg.HES, pg.QE), (pg.GBM, pg.LAW), (pg.HES, _ffi.HH_BROADIE_KAYA)):
                if (dyn, strat) != (src.dynamics, src.strategy):
                    lognormal_euler = src.kind == _ffi.HH_SOURCE_EULER and dyn == pg.GBM  # that walk holds no variance
                    expect(S, M, C.byref(_ffi.make_config(dyn, strat, n, steps, seeds=pg.seeds_for(n))), UNS,
                           "no variance" if lognormal_euler else " needs ")
            expect(S, C.byref(src.model(T=0.0)), Cc, INV, "model scalars", named=False)
        # the walks that hold no variance: the source kind, and lognormal dynamics on the Euler source
        for src in ps.no_variance_sources():
            s, m, c = src.source(), src.model(), src.config(n, steps)
            expect(C.byref(s), C.byref(m), C.byref(c), UNS, "no variance")
        src = SOURCES[0]
        s, m, c = src.source(), src.model(), src.config(n, steps)
        unknown = _ffi.make_path_source(6)
        expect(C.byref(unknown), C.byref(m), C.byref(c), INV, "unknown source kind 6")
        unknown.kind = -1
        expect(C.byref(unknown), C.byref(m), C.byref(c), INV, "unknown source kind -1")
        expect(C.byref(s), C.byref(m), C.byref(src.config(8, 65535)), INV, "6553", named=False)
        lib, h = ctx.lib, ctx.handle
        assert lib.hh_mc_path_states(h, C.byref(s), C.byref(m), C.byref(c), 1, None, 0, None) == INV
        assert "NULL argument" in lib.hh_last_error(h).decode()
        assert lib.hh_lsm_solve_path_states(h, C.byref(s), C.byref(m), C.byref(c), 1, 3, 0.99, None, None, None, None, None) == INV
        assert "NULL argument" in lib.hh_last_error(h).decode()
        for degree, D, cp in ((0, 0.99, -1.0), (9, 0.99, -1.0), (3, 0.0, -1.0), (3, float("nan"), -1.0), (3, 0.99, 0.5)):
            mm = src.model(cp=cp)
            rc = lib.hh_lsm_solve_path_states(h, C.byref(s), C.byref(mm), C.byref(c), 1, degree, D, C.byref(out), None, None, None, None)
            assert rc == INV and "LSM" in lib.hh_last_error(h).decode()
        # the schedule is checked before the induction's scalars, those before the source's own checks
        rc = lib.hh_lsm_solve_path_states(h, C.byref(s), C.byref(m), C.byref(src.config(n, steps, n_partials=2)), 5, 0, 0.99,
                                          C.byref(out), None, None, None, None)
        assert rc == INV and "exercise_every" in lib.hh_last_error(h).decode()
        rc = lib.hh_lsm_solve_path_states(h, C.byref(s), C.byref(m), C.byref(src.config(n, steps, n_partials=2)), 3, 0, 0.99,
                                          C.byref(out), None, None, None, None)
        assert rc == INV and "LSM" in lib.hh_last_error(h).decode()
        rc = lib.hh_lsm_solve_path_states(h, C.byref(s), C.byref(src.model(strike=float("inf"))), C.byref(c), 3, 3, 0.99,
                                          C.byref(out), None, None, None, None)
        assert rc == INV and "strike" in lib.hh_last_error(h).decode()
        # the descriptor of hh_lsm_solve_states: the new kind takes two state rows, an unknown kind stays what it was
        import torch
        dev = torch.zeros(3 * 2 * 64, dtype=torch.float64, device="cuda")
        for d, text in ((ps.desc(-1.0, 100.0, n_states=1), "n_states"), (ps.desc(-1.0, 100.0, n_states=3), "n_states"),
                        (ps.desc(-1.0, 100.0, kind=2), "unknown descriptor kind 2"), (ps.desc(-1.0, 100.0, kind=-1), "unknown descriptor kind -1"),
                        (ps.desc(-1.0, float("nan")), "strike"), (ps.desc(2.0, 100.0), "LSM")):
            rc = lib.hh_lsm_solve_states(h, C.byref(d), dev.data_ptr(), 64, 2, 3, 0.99, C.byref(out), None, None, None)
            assert rc == INV and text in lib.hh_last_error(h).decode(), text
        assert ctx.read_timings() == []  # nothing was launched
        # … and the context solves: one timing slot for the rows
        assert np.all(np.isfinite(ps.path_states(ctx, src, m, c, 3)))
        assert len(ctx.read_timings()) == 1
    finally:
        ctx.enable_timing(False)
