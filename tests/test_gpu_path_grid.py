"""Date rows of the log-spot path family (hh_mc_path_grid) and American / Bermudan exercise on them (hh_lsm_solve_path).

BIT FOR BIT, per source: the rows against the five statistics of the source's hh_mc_path_stats* call — kernels that are
held path by path to 50-digit restatements — on every divisor of 12 steps with and without the start; a coarser grid
against the rows of the finest; the Euler source against hh_euler_grid, which is pinned to the oracle; a constant
local-volatility table, λ = 0 under Bates and under Merton against the member of the family they reduce to; one wave
against many, and path_offset; hh_lsm_solve_path against hh_lsm_solve_grid on the grid it handed back, in both induction
forms.  EVERY ROW of the QE and Bates grids against the 50-digit walks of qe_cases.py / bates_cases.py — the restatements
that expose the log spot after every step — on those modules' own models, seeds, shapes and bars.  PRICES: one exercise date against the source's European solve; American against European on the same draws; the
reference's put on a constant table against a 1000-step tree; a Bermudan schedule between the two."""
import ctypes as C
import math

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from oracle import analytic
from tests import path_grid_cases as pg

pytestmark = pytest.mark.gpu

SOURCES = pg.identity_sources()
IDS = [s.name for s in SOURCES]
BIG = 513
_G1 = {}


def finest(ctx, src, anti):
    """G1: the 13 rows of BIG trajectories at exercise_every = 1 — computed once per source and mirror, never changed"""
    key = (src.name, anti)
    if key not in _G1:
        g = pg.path_grid(ctx, src, src.model(), src.config(BIG, pg.STEPS, anti), 1)
        g.setflags(write=False)
        _G1[key] = g
    return _G1[key]


# ---- 1. the rows are the trajectories of the statistics kernels -----------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("src", SOURCES, ids=IDS)
def test_rows_against_the_statistics(hhlib, src, anti):
    G1 = finest(hhlib, src, anti)
    assert G1.shape == (pg.STEPS + 1, BIG * (1 + anti)) and np.all(np.isfinite(G1)) and np.all(G1 > 0.0)
    m, c = src.model(), src.config(BIG, pg.STEPS, anti)
    assert np.all(G1[0] == m.S0)
    for every in pg.DIVISORS:
        for start in (0, 1):
            stats = src.stats(hhlib, m, c, every, start)
            rows = ([G1[0]] if start else []) + [G1[k] for k in range(every, pg.STEPS + 1, every)]
            total = rows[0].copy()
            for r in rows[1:]:  # one rounded addition per date, in date order
                total = total + r
            where = f"{src.name} every={every} start={start}"
            assert np.array_equal(stats[_ffi.HH_STAT_S_T], G1[pg.STEPS]), where
            assert np.array_equal(stats[_ffi.HH_STAT_MAX_S], np.max(rows, axis=0)), where
            assert np.array_equal(stats[_ffi.HH_STAT_MIN_S], np.min(rows, axis=0)), where
            assert np.array_equal(stats[_ffi.HH_STAT_SUM_S], total), where


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("src", SOURCES, ids=IDS)
def test_a_coarser_grid_is_rows_of_the_finest(hhlib, src, anti):
    G1 = finest(hhlib, src, anti)
    m, c = src.model(), src.config(BIG, pg.STEPS, anti)
    for every in pg.EVERY:
        g = pg.path_grid(hhlib, src, m, c, every)
        assert g.shape[0] == pg.STEPS // every + 1 and np.array_equal(g, G1[::every]), (src.name, every)


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("src", SOURCES, ids=IDS)
def test_one_wave_and_many_give_the_same_columns_and_path_offset_is_not_read(hhlib, src, anti):
    G1 = finest(hhlib, src, anti)
    seeds = pg.seeds_for(BIG, 17)
    for n in pg.SIZES:
        c = src.config(n, pg.STEPS, anti, seeds=seeds[:n], path_offset=(n * 1000003) if n != 64 else 0)
        for every in pg.EVERY:
            g = pg.path_grid(hhlib, src, src.model(), c, every)
            for mem in range(1 + anti):
                assert np.array_equal(g[:, mem * n:(mem + 1) * n], G1[::every, mem * BIG:mem * BIG + n]), (src.name, n, every, mem)


# ---- 2. against the other members of the family ---------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [12, 7])  # 7: the scalar-noise forms half-read their last Philox block
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("src", SOURCES[:3], ids=IDS[:3])
def test_the_euler_source_is_hh_euler_grid(hhlib, src, anti, steps):
    m, c = src.model(), src.config(BIG, steps, anti)
    want = np.full((steps + 1, pg.n_total(c)), np.nan)
    hhlib.check(hhlib.lib.hh_euler_grid(hhlib.handle, C.byref(m), C.byref(c), _ffi.HH_PATH_SPOT, want.ctypes.data, None, 0, None))
    assert np.array_equal(pg.path_grid(hhlib, src, m, c, 1), want)


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("shape", [(1, 64), (16, 128)])
def test_a_constant_table_is_the_euler_source(hhlib, shape, anti):
    s0 = 0.2
    lv, eu = pg.localvol(*shape, sigma=s0), pg.euler(params=dict(pg.FLAT, sigma=s0))
    c = lv.config(BIG, pg.STEPS, anti)
    for every in (1, 4):
        assert np.array_equal(pg.path_grid(hhlib, lv, lv.model(), c, every), pg.path_grid(hhlib, eu, eu.model(), c, every))


@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("mart", [0, 1])
def test_bates_without_jumps_is_the_qe_source(hhlib, mart, anti):
    b, q = pg.bates(mart, lam=0.0), pg.qe(mart)
    c = q.config(BIG, pg.STEPS, anti)
    assert np.array_equal(pg.path_grid(hhlib, b, b.model(), c, 1), pg.path_grid(hhlib, q, q.model(), c, 1))


@pytest.mark.parametrize("anti", [0, 1])
def test_merton_without_jumps_is_the_euler_source(hhlib, anti):
    j, eu = pg.merton(lam=0.0), pg.euler(params=dict(pg.FLAT, sigma=0.2))
    c = eu.config(BIG, pg.STEPS, anti)
    assert np.array_equal(pg.path_grid(hhlib, j, j.model(), c, 1), pg.path_grid(hhlib, eu, eu.model(), c, 1))


# ---- 3. the induction behind the grid -------------------------------------------------------------------------------------

@pytest.mark.parametrize("src", [SOURCES[i] for i in (1, 3, 5, 7, 9, 10)], ids=[IDS[i] for i in (1, 3, 5, 7, 9, 10)])
def test_lsm_is_hh_lsm_solve_grid_on_the_grid_handed_back(hhlib, src):
    import torch
    n, steps, every, degree, anti = 3001, 24, 3, 3, 1
    m, c = src.model(strike=102.0), src.config(n, steps, anti)
    D = math.exp(-m.r_drift * m.T * every / steps)
    res, tau, val, grid = pg.lsm_path(hhlib, src, m, c, every, degree, D)
    assert np.array_equal(grid, pg.path_grid(hhlib, src, m, c, every))
    assert res.n_paths_total == 2 * n and res.rows_regressed + res.rows_skipped > 0
    assert tau.min() >= 1 and tau.max() <= steps // every  # exercise dates, not steps
    dev = torch.from_numpy(grid).cuda()
    torch.cuda.synchronize()
    res2, tau2, val2 = _ffi.hh_lsm_result(), np.zeros_like(tau), np.zeros_like(val)
    hhlib.check(hhlib.lib.hh_lsm_solve_grid(hhlib.handle, C.byref(m), dev.data_ptr(), grid.shape[1], steps // every, degree, D,
                                            C.byref(res2), tau2.ctypes.data, val2.ctypes.data))
    assert (res2.price, res2.std_error) == (res.price, res.std_error)
    assert np.array_equal(tau2, tau) and np.array_equal(val2, val)
    out = {}
    try:
        for form in (_ffi.HH_LSM_FORM_PERSISTENT, _ffi.HH_LSM_FORM_PER_DATE):
            hhlib.set_option(_ffi.HH_OPT_LSM_FORM, form)
            out[form] = pg.lsm_path(hhlib, src, m, c, every, degree, D, want_grid=False)
    finally:
        hhlib.set_option(_ffi.HH_OPT_LSM_FORM, _ffi.HH_LSM_FORM_AUTO)
    for form, (r, t, v, _) in out.items():
        assert r.form == form
        assert (r.price, r.std_error, r.rows_regressed, r.rows_skipped) == \
               (res.price, res.std_error, res.rows_regressed, res.rows_skipped)
        assert np.array_equal(t, tau) and np.array_equal(v, val)


# ---- 4. prices ------------------------------------------------------------------------------------------------------------

PRICED = pg.price_sources()
PRICED_IDS = [s.name for s in PRICED]
N_PRICE, DEGREE = 200_000, 3


def _schedule(src):
    """(steps, exercise_every) of 50 exercise dates: 100 steps for the discretised sources, 50 exact-in-law spans for VG"""
    return (50, 1) if src.kind == _ffi.HH_SOURCE_VG else (100, 2)


def _price_case(src, cp):
    steps, every = _schedule(src)
    m = src.model(T=1.0, strike=100.0, cp=cp)
    c = src.config(N_PRICE, steps, 0, seeds=np.arange(1, N_PRICE + 1, dtype=np.uint64))
    return m, c, steps, every


@pytest.mark.parametrize("src", PRICED, ids=PRICED_IDS)
def test_one_exercise_date_is_the_european_solve(hhlib, src):
    """exercise_every = n_steps: date_discount times the mean payoff at expiry — the source's vanilla on the same seeds, up
    to the order of the summation: 2·10^5 terms of like sign, each sum within n·2^-53 ≈ 2·10^-11 of the exact one at worst
    and, added pairwise and in blocks as both are, far below 10^-12."""
    for cp in (-1.0, 1.0):
        m, c, steps, _ = _price_case(src, cp)
        res, _, _, _ = pg.lsm_path(hhlib, src, m, c, steps, DEGREE, m.discount, want_grid=False, want_stops=False)
        eu = src.vanilla(hhlib, m, c)
        print(f"\n{src.name} cp={cp:+.0f}: one date {res.price!r}, European {eu.price!r}")
        assert res.price == pytest.approx(eu.price, rel=1e-12)
        assert res.std_error == pytest.approx(eu.std_error, rel=1e-9)


@pytest.mark.parametrize("src", PRICED, ids=PRICED_IDS)
def test_american_against_european_on_the_same_draws(hhlib, src):
    """The argument and the bounds of test_gpu_lsm_euler.py::test_heston_american_against_european_on_the_same_draws: the
    put is worth at least the European one less 3 combined standard errors; the call (r >= 0, no dividends — early
    exercise is never optimal under any of these models: S·e^{-rt} is a martingale in each) is the European one within 3
    combined standard errors + 1 % of its price."""
    for cp in (-1.0, 1.0):
        m, c, steps, every = _price_case(src, cp)
        D = math.exp(-m.r_drift * m.T * every / steps)
        am, _, _, _ = pg.lsm_path(hhlib, src, m, c, every, DEGREE, D, want_grid=False, want_stops=False)
        eu = src.vanilla(hhlib, m, c)
        se = math.hypot(am.std_error, eu.std_error)
        print(f"\n{src.name} cp={cp:+.0f}: American {am.price:.5f} ± {am.std_error:.5f}, European {eu.price:.5f} ± {eu.std_error:.5f}")
        if cp < 0:
            assert am.price >= eu.price - 3 * se
        else:
            assert abs(am.price - eu.price) <= 3 * se + 0.01 * eu.price


@pytest.mark.parametrize("src", PRICED, ids=PRICED_IDS)
def test_a_bermudan_put_lies_between_the_european_and_the_american(hhlib, src):
    """One seed set: 50 dates >= 5 dates - 3 combined standard errors, 5 dates >= European - 3 combined standard errors —
    a holder with more dates can do whatever one with fewer does (the estimates' policy losses and foresight biases are
    those of the test above: within the standard errors at this size)."""
    m, c, steps, every = _price_case(src, -1.0)

    def put(e):
        D = math.exp(-m.r_drift * m.T * e / steps)
        return pg.lsm_path(hhlib, src, m, c, e, DEGREE, D, want_grid=False, want_stops=False)[0]

    p50, p5, eu = put(every), put(every * 10), src.vanilla(hhlib, m, c)
    print(f"\n{src.name}: 50 dates {p50.price:.5f} ± {p50.std_error:.5f}, 5 dates {p5.price:.5f} ± {p5.std_error:.5f}, "
          f"European {eu.price:.5f} ± {eu.std_error:.5f}")
    assert p50.price >= p5.price - 3 * math.hypot(p50.std_error, p5.std_error)
    assert p5.price >= eu.price - 3 * math.hypot(p5.std_error, eu.std_error)


def test_reference_put_on_a_constant_table_against_crr(hhlib):
    """american_options.jl's put — S0 = K = 100, r = 0.05, σ = 0.2, T = 1 — on a constant local-volatility table: 5·10^4
    antithetic pairs, 100 steps, degree 5, against the 1000-step tree at the reference's own rtol 0.02
    (test_gpu_lsm_euler.py::test_lognormal_euler_reference_put_vs_crr)."""
    n, steps = 50_000, 100
    src = pg.localvol(16, 128, sigma=0.2, r=0.05)
    m = src.model(T=1.0, strike=100.0, cp=-1.0)
    c = src.config(n, steps, 1, seeds=np.random.default_rng(12345).integers(0, 2**63, n).astype(np.uint64))
    res, _, _, _ = pg.lsm_path(hhlib, src, m, c, 1, 5, math.exp(-0.05 / steps), want_grid=False, want_stops=False)
    want = analytic.crr_price(100, 100, 0.05, 0.2, 1.0, 1000, cp=-1.0)
    print(f"\nLSM {res.price:.5f} ± {res.std_error:.5f}, CRR {want:.5f}")
    assert res.price == pytest.approx(want, rel=0.02)


# ---- 5. the host mirror ---------------------------------------------------------------------------------------------------

def test_host_mirror(hhlib):
    import hedgehog_jl_amd as hh
    ref, exp = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
    n, steps, every = 20_000, 24, 4
    cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64), variance_reduction=hh.Antithetic())
    put = hh.VanillaOption(100.0, exp, hh.American(), hh.Put(), hh.Spot())
    mkt = hh.VarianceGammaInputs(ref, 0.03, 100.0, 0.2, -0.3, 0.5)
    method = hh.LSM(hh.VarianceGammaDynamics(), hh.VarianceGammaExact(), cfg, 3)
    sol = hh.solve(hh.PricingProblem(put, mkt), method, spot_paths=True, exercise_every=every)
    assert isinstance(sol, hh.LSMSolution) and sol.spot_paths.shape == (steps // every + 1, 2 * n)
    tau, _ = sol.stopping_info
    assert tau.min() >= 1 and tau.max() <= steps // every
    paths = hh.simulate_spot_paths(hh.PricingProblem(put, mkt), method.mc_method, exercise_every=every)
    assert np.array_equal(paths.spot, sol.spot_paths) and paths.times[-1] == 1.0 and paths.times.size == steps // every + 1
    european = hh.VanillaOption(100.0, exp, hh.European(), hh.Put(), hh.Spot())
    eu = hh.solve(hh.PricingProblem(european, mkt), method.mc_method)  # the law at expiry: other draws
    assert sol.price >= eu.price - 3 * math.hypot(sol.std_error, eu.std_error)
    # the Euler source under a Bermudan schedule: rows of hh_euler_grid
    bs = hh.BlackScholesInputs(ref, 0.03, 100.0, 0.2)
    em = hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg, 3)
    coarse = hh.solve(hh.PricingProblem(put, bs), em, spot_paths=True, path_state="spot", exercise_every=every)
    fine = hh.simulate_euler_paths(hh.PricingProblem(put, bs), em.mc_method)
    assert np.array_equal(coarse.spot_paths, fine.spot[::every])


# ---- 6. refusals: all of them before any launch ---------------------------------------------------------------------------

def test_every_refusal_comes_back_before_a_launch(hhlib):
    ctx = hhlib
    n, steps = 300, 12
    INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
    grid = np.empty((steps + 1, n))
    out = _ffi.hh_lsm_result()

    def both(source, m, c, every=1, degree=3, D=0.99):
        a = ctx.lib.hh_mc_path_grid(ctx.handle, source, m, c, every, grid.ctypes.data, 0, None)
        ta = ctx.lib.hh_last_error(ctx.handle).decode()
        b = ctx.lib.hh_lsm_solve_path(ctx.handle, source, m, c, every, degree, D, C.byref(out), None, None, None)
        return (a, ta), (b, ctx.lib.hh_last_error(ctx.handle).decode())

    def expect(source, m, c, code, text, named=True, **kw):
        """named: the message names the entry point (the scalar checks of the induction speak as "LSM", as hh_lsm_solve_euler's)"""
        for who, (rc, msg) in zip(("hh_mc_path_grid", "hh_lsm_solve_path"), both(source, m, c, **kw)):
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
                admitted = (dyn, strat) == (src.dynamics, src.strategy) or (src.kind == _ffi.HH_SOURCE_EULER and strat == pg.EM)
                if not admitted:
                    expect(S, M, C.byref(_ffi.make_config(dyn, strat, n, steps, seeds=pg.seeds_for(n))), UNS, " needs ")
            expect(S, C.byref(src.model(T=0.0)), Cc, INV, "model scalars", named=False)
        src = SOURCES[0]
        s, m, c = src.source(), src.model(), src.config(n, steps)
        unknown = _ffi.make_path_source(6)
        expect(C.byref(unknown), C.byref(m), C.byref(c), INV, "unknown source kind 6")
        unknown.kind = -1
        expect(C.byref(unknown), C.byref(m), C.byref(c), INV, "unknown source kind -1")
        # more dates than the induction's grid has rows for: 65535 steps, every one a date
        expect(C.byref(s), C.byref(m), C.byref(src.config(8, 65535)), INV, "6553", named=False)
        rc = ctx.lib.hh_lsm_solve_path(ctx.handle, C.byref(s), C.byref(m), C.byref(c), 1, 3, 0.99, None, None, None, None)
        assert rc == INV and "NULL argument" in ctx.lib.hh_last_error(ctx.handle).decode()
        for degree, D in ((0, 0.99), (9, 0.99), (3, 0.0), (3, float("nan"))):
            rc = ctx.lib.hh_lsm_solve_path(ctx.handle, C.byref(s), C.byref(m), C.byref(c), 1, degree, D, C.byref(out), None, None, None)
            assert rc == INV and "LSM" in ctx.lib.hh_last_error(ctx.handle).decode()
        assert ctx.read_timings() == []  # nothing was launched
        # … and the context solves: one timing slot for a grid
        assert np.all(np.isfinite(pg.path_grid(ctx, src, m, c, 3)))
        assert len(ctx.read_timings()) == 1
    finally:
        ctx.enable_timing(False)


# ---- 7. every row against the 50-digit restatements that expose the per-date states ---------------------------------------

def _rows_against_the_walks(ctx, worst, family, name, case, src_of, config, runs_of, n_steps, every, anti, mart, reference):
    """Row j of the grid at exercise_every = m is exp(x) after step j·m: S_T of the restatement's rows over the first j·m
    steps monitored at j·m alone, at the module's own bar, euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A)."""
    from tests import euler_tangent_cases as etc
    src = src_of(mart, case)
    m = src.model(T=case["T"])
    grid = pg.path_grid(ctx, src, m, config(anti), every)
    n = grid.shape[1] // (1 + anti)
    assert np.all(grid[0] == case["S0"])
    runs = runs_of()[:1 + anti]
    bad = []
    for j in range(1, n_steps // every + 1):
        upto = j * every
        cut = [[(xs_mp[:upto], v_mp, xs_64[:upto], v_64) for xs_mp, v_mp, xs_64, v_64 in member] for member in runs]
        ref = reference(case, cut, upto, 0)
        bars = etc.path_bar(ref["e64"], ref["A"])
        for mem in range(1 + anti):
            for i in range(n):
                bad.append(worst.check(f"{family} row", grid[j][mem * n + i], ref["want"][mem][i][_ffi.HH_STAT_S_T],
                                       bars[mem][i][_ffi.HH_STAT_S_T],
                                       f"{name} {n_steps} steps every={every} anti={anti} mart={mart} row {j} member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


@pytest.fixture(scope="module")
def worst_rows():
    from tests import euler_tangent_cases as etc
    w = etc.Worst("date rows (device)")
    yield w
    w.report()


@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1), (5, 1), (6, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["feller", "low_v0"])
def test_qe_rows_against_the_50_digit_walk(hhlib, oracle, worst_rows, name, shape, anti, mart):
    """qe_cases' own models, seeds (257 trajectories) and shapes; the walks are test_gpu_qe.py's, computed once a session"""
    from tests import qe_cases as qc
    from tests import test_gpu_qe as tq
    assert shape in qc.PATH_SHAPES and name in qc.MODELS
    n_steps, every = shape
    case, seeds = qc.MODELS[name], qc.path_seeds()
    Z = tq.cached(("Z", n_steps), lambda: qc.step_normals(oracle, seeds, n_steps))
    U = tq.cached(("U", n_steps), lambda: qc.step_uniforms(oracle, seeds, n_steps))
    _rows_against_the_walks(hhlib, worst_rows, "qe", name, case, lambda mart, case: pg.qe(mart, case, f"qe-{name}"),
                            lambda anti: qc.config_of(qc.PATH_N, n_steps, seeds, anti),
                            lambda: tq.cached(("runs", name, n_steps, mart), lambda: qc.walks(case, n_steps, Z, U, 1, mart)[0]),
                            n_steps, every, anti, mart, qc.reference)


@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1), (5, 1), (6, 1), (6, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["feller", "low_v0"])
def test_bates_rows_against_the_50_digit_walk(hhlib, oracle, worst_rows, name, shape, anti, mart):
    """bates_cases' own models, jumps (λ·dt = 0.9), seeds and shapes; the walks are test_gpu_bates.py's"""
    from tests import bates_cases as bt
    from tests import test_gpu_bates as tb
    assert shape in bt.PATH_SHAPES and name in bt.MODELS
    n_steps, every = shape
    case, seeds = bt.path_case(name, n_steps), bt.path_seeds()
    d = tb.cached(("d", n_steps), lambda: bt.draws(oracle, seeds, n_steps))
    N = tb.cached(("N", name, n_steps), lambda: bt.counts(d["UJ"], bt.path_mean(case, n_steps)))

    def src_of(mart, case):
        return pg.bates(mart, lam=case["lam"], case=case, name=f"bates-{name}")

    _rows_against_the_walks(hhlib, worst_rows, "bates", name, case, src_of,
                            lambda anti: bt.config_of(bt.PATH_N, n_steps, seeds, anti),
                            lambda: tb.cached(("runs", name, n_steps, mart), lambda: bt.walks(case, n_steps, d, N, 1, mart)[0]),
                            n_steps, every, anti, mart, bt.reference)
