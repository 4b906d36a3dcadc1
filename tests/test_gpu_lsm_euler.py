"""Euler–Maruyama path grids (hh_euler_grid) and LSM on them (hh_lsm_solve_euler), the opt-in path source of
LognormalDynamics / HestonDynamics + EulerMaruyama: every row against the CPU oracle, the last row against the
production kernel, the induction against the numpy oracle and against itself, and the host mirror."""
import ctypes as C
import math

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from oracle import analytic, lsm_oracle
from tests import oracle_ffi as o

pytestmark = pytest.mark.gpu

GBM, HES = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON
EM = _ffi.HH_EULER_MARUYAMA
SPOT, LOG = _ffi.HH_PATH_SPOT, _ffi.HH_PATH_LOG
H252 = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03)
# the parameter set the reference's own Heston test runs (test_gpu_parity.py): 2κθ = 0.024 < σ² = 0.36,
# the Feller condition fails and the Euler variance goes negative on many paths
Q2 = dict(S0=100.0, V0=1.5, kappa=0.04, theta=0.3, sigma=-0.6, rho=0.04, r=0.05)


def seeds_for(n, salt=0):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt)


def model(dyn, params, T, strike=100.0, cp=-1.0):
    p = dict(params)
    if dyn == GBM:
        p.update(V0=0.0, kappa=0.0, theta=0.0, rho=0.0, sigma=0.25)
    return o.make_model(**p, T=T, strike=strike, cp=cp)


def euler_grid(ctx, m, c, state, want_var=False):
    ntot = c.n_paths * (2 if c.antithetic else 1)
    spot = np.full((c.n_steps + 1, ntot), np.nan)
    var = np.full_like(spot, np.nan) if want_var else None
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_euler_grid(ctx.handle, C.byref(m), C.byref(c), state, spot.ctypes.data,
                                    var.ctypes.data if want_var else None, 0, C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return spot, var


def lsm_euler(ctx, m, c, state, degree, D, want_grid=True):
    ntot = c.n_paths * (2 if c.antithetic else 1)
    tau, val = np.zeros(ntot, dtype=np.int32), np.zeros(ntot)
    grid = np.zeros((c.n_steps + 1, ntot)) if want_grid else None
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve_euler(ctx.handle, C.byref(m), C.byref(c), state, degree, D, C.byref(res),
                                         tau.ctypes.data, val.ctypes.data,
                                         grid.ctypes.data if want_grid else None))
    return res, tau, val, grid


# ---- 1. every row against the CPU oracle -------------------------------------------------------------------------

def check_rows_against_oracle(ctx, oracle, dyn, params, split, anti, state, n, N):
    """Draws are keyed by (seed, step): row k of an N-step grid is the terminal of the oracle's k-step solve over
    T' = k·dt on the same seeds — dt = 1/64 is the same double both ways (T = N/64, T' = k/64)."""
    seeds = seeds_for(n, N)
    m = model(dyn, params, T=N / 64)
    c = o.make_config(dyn, EM, n, N, antithetic=anti, em_split=split, seeds=seeds)
    spot, var = euler_grid(ctx, m, c, state, want_var=dyn == HES)
    x0 = math.log(m.S0)
    assert np.all(spot[0] == (x0 if state == LOG else m.S0))
    for k in range(1, N + 1):
        mk = model(dyn, params, T=k / 64)
        ck = o.make_config(dyn, EM, n, k, antithetic=anti, em_split=split, seeds=seeds)
        _, term, _ = oracle.mc_solve(mk, ck)
        if state == SPOT:
            np.testing.assert_allclose(spot[k], term, rtol=1e-11, atol=0, err_msg=f"row {k}")
        else:  # the log state: |Δx| = |ΔS / S|
            np.testing.assert_allclose(spot[k], np.log(term), rtol=0, atol=1e-11, err_msg=f"row {k}")
    if state == LOG:
        # the same states as the spot grid, before its exp: a log-row error far below the oracle's 1e-11 shows here
        # (device exp and numpy exp of the same double differ by an ulp or two)
        spot_rows, _ = euler_grid(ctx, m, c, SPOT)
        np.testing.assert_allclose(np.exp(spot), spot_rows, rtol=1e-15, atol=0)
    if dyn == HES:
        assert np.all(var[0] == m.V0) and np.all(np.isfinite(var))
        alone, _ = euler_grid(ctx, m, c, state)  # the variance rows change nothing in the spot rows
        np.testing.assert_array_equal(alone, spot)


@pytest.mark.parametrize("state", [SPOT, LOG])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("dyn", [GBM, HES])
def test_every_row_matches_the_oracle(hhlib, oracle, dyn, split, anti, state):
    check_rows_against_oracle(hhlib, oracle, dyn, H252, split, anti, state, n=1000, N=64)


@pytest.mark.parametrize("dyn,params,split,anti,state,n,N", [
    (GBM, H252, 1, 0, SPOT, 257, 1),     # one step: half a Philox pair
    (GBM, H252, 1, 1, LOG, 300, 7),      # odd: the last step takes z1 of a pair whose z2 is unused
    (HES, H252, 0, 1, SPOT, 513, 1),
    (HES, H252, 1, 0, LOG, 255, 9),
    (HES, Q2, 1, 1, SPOT, 1000, 33),     # Feller violated: the clip at v+ = 0 on many paths
    (HES, Q2, 0, 0, LOG, 777, 20),
])
def test_rows_on_ragged_and_odd_shapes(hhlib, oracle, dyn, params, split, anti, state, n, N):
    check_rows_against_oracle(hhlib, oracle, dyn, params, split, anti, state, n, N)


# ---- 2. the last row against the production kernel ---------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("dyn", [GBM, HES])
def test_last_row_is_the_terminal_of_hh_mc_solve_bit_for_bit(hhlib, dyn, split, anti):
    n, N = 3001, 50
    m = model(dyn, H252, T=1.0)
    c = o.make_config(dyn, EM, n, N, antithetic=anti, em_split=split, seeds=seeds_for(n, 5))
    spot, _ = euler_grid(hhlib, m, c, SPOT)
    term = np.zeros(n * (2 if anti else 1))
    res = _ffi.hh_result()
    hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(res), term.ctypes.data))
    np.testing.assert_array_equal(spot[N], term)


# ---- 3. LSM against the oracle, and against hh_lsm_solve_grid -----------------------------------------------------

@pytest.mark.parametrize("dyn,state,anti,cp,K,degree,n,N", [
    (HES, SPOT, 0, -1.0, 100.0, 5, 3000, 30),
    (HES, SPOT, 1, -1.0, 110.0, 3, 1025, 7),
    (HES, LOG, 0, -1.0, 4.7, 4, 3000, 30),       # the reference as run: payoff and regression on log S
    (HES, LOG, 1, 1.0, 4.5, 3, 700, 12),
    (GBM, SPOT, 1, 1.0, 100.0, 4, 3000, 30),
    (GBM, LOG, 0, -1.0, 4.65, 2, 700, 1),
])
def test_lsm_matches_oracle(hhlib, dyn, state, anti, cp, K, degree, n, N):
    import torch
    m = model(dyn, H252, T=0.75, strike=K, cp=cp)
    c = o.make_config(dyn, EM, n, N, antithetic=anti, seeds=seeds_for(n, 11))
    D = math.exp(-H252["r"] * 0.75 / N)
    res, tau, val, grid = lsm_euler(hhlib, m, c, state, degree, D)
    spot, _ = euler_grid(hhlib, m, c, state)
    np.testing.assert_array_equal(grid, spot)
    ref = lsm_oracle.lsm_solve(grid, K, cp, D, degree)
    assert res.n_paths_total == grid.shape[1]
    assert res.rows_regressed == ref["steps_regressed"]
    assert res.rows_regressed + res.rows_skipped == max(N - 1, 0)
    same = tau == ref["stop_time"]
    assert same.mean() >= 0.998
    scale = abs(grid).max()
    np.testing.assert_allclose(val[same], ref["stop_value"][same], rtol=1e-12, atol=1e-13 * scale)
    assert res.price == pytest.approx(ref["price"], rel=2e-4 if not same.all() else 1e-11)
    assert res.std_error == pytest.approx(ref["std_error"], rel=1e-3)
    # the same induction on the same grid uploaded by the caller: bit for bit
    dev = torch.from_numpy(grid).cuda()
    torch.cuda.synchronize()
    res2 = _ffi.hh_lsm_result()
    tau2, val2 = np.zeros_like(tau), np.zeros_like(val)
    hhlib.check(hhlib.lib.hh_lsm_solve_grid(hhlib.handle, C.byref(m), dev.data_ptr(), grid.shape[1], N, degree,
                                            D, C.byref(res2), tau2.ctypes.data, val2.ctypes.data))
    assert (res2.price, res2.std_error) == (res.price, res.std_error)
    np.testing.assert_array_equal(tau2, tau)
    np.testing.assert_array_equal(val2, val)


# ---- 4. the two induction forms ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dyn,state,n,N,anti,degree", [
    (HES, SPOT, 3000, 30, 1, 5),
    (HES, LOG, 300_000, 12, 0, 4),
    (GBM, SPOT, 140_000, 12, 1, 3),
    (HES, SPOT, 1_100_000, 4, 1, 3),   # 2.2·10^6 trajectories > 2^21: both settings run per date
])
def test_one_launch_and_launch_per_date_agree_bit_for_bit(hhlib, dyn, state, n, N, anti, degree):
    K = 4.65 if state == LOG else 105.0
    m = model(dyn, H252, T=0.5, strike=K, cp=-1.0)
    c = o.make_config(dyn, EM, n, N, antithetic=anti, seeds=np.arange(1, n + 1, dtype=np.uint64))
    D = math.exp(-H252["r"] * 0.5 / N)
    out = {}
    try:
        for form in (_ffi.HH_LSM_FORM_PERSISTENT, _ffi.HH_LSM_FORM_PER_DATE):
            hhlib.set_option(_ffi.HH_OPT_LSM_FORM, form)
            out[form] = lsm_euler(hhlib, m, c, state, degree, D, want_grid=False)
    finally:
        hhlib.set_option(_ffi.HH_OPT_LSM_FORM, _ffi.HH_LSM_FORM_AUTO)
    (ra, ta, va, _), (rb, tb, vb, _) = out[_ffi.HH_LSM_FORM_PERSISTENT], out[_ffi.HH_LSM_FORM_PER_DATE]
    ntot = n * (2 if anti else 1)
    assert ra.form == (_ffi.HH_LSM_FORM_PER_DATE if ntot > 2**21 else _ffi.HH_LSM_FORM_PERSISTENT)
    assert rb.form == _ffi.HH_LSM_FORM_PER_DATE
    np.testing.assert_array_equal(ta, tb)
    np.testing.assert_array_equal(va, vb)
    assert (ra.price, ra.std_error, ra.rows_regressed, ra.rows_skipped) == \
           (rb.price, rb.std_error, rb.rows_regressed, rb.rows_skipped)


# ---- 5. lognormal Euler against the exact law ----------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
def test_lognormal_euler_is_the_exact_gbm_grid(hhlib, anti):
    """The log-Euler step of GBM is exact in law, and both grids draw the same kDomEuler normals per (seed, step):
    the Euler spot grid is lsm_oracle.gbm_grid up to rounding, and the LSM prices agree as test_gpu_lsm's do."""
    n, N, S0, K, r, sigma, T, degree = 3000, 30, 100.0, 105.0, 0.05, 0.25, 0.75, 4
    seeds = seeds_for(n, 17)
    m = o.make_model(S0=S0, sigma=sigma, r=r, T=T, strike=K, cp=-1.0)
    D = math.exp(-r * T / N)
    ce = o.make_config(GBM, EM, n, N, antithetic=anti, seeds=seeds)
    re, te, _, grid = lsm_euler(hhlib, m, ce, SPOT, degree, D)
    np.testing.assert_allclose(grid, lsm_oracle.gbm_grid(seeds, N, S0, r, sigma, T, anti), rtol=1e-12)
    cx = o.make_config(GBM, _ffi.HH_EXACT_LAW, n, N, antithetic=anti, seeds=seeds)
    rx = _ffi.hh_lsm_result()
    tx = np.zeros_like(te)
    hhlib.check(hhlib.lib.hh_lsm_solve(hhlib.handle, C.byref(m), C.byref(cx), degree, D, C.byref(rx),
                                       tx.ctypes.data, None, None))
    same = te == tx
    assert same.mean() >= 0.998
    assert re.price == pytest.approx(rx.price, rel=2e-4 if not same.all() else 1e-11)


def test_lognormal_euler_reference_put_vs_crr():
    """american_options.jl's put (rtol 0.02) on Euler paths, through the host mirror."""
    ref = hh.Date(2020, 1, 1)
    expiry = hh.add_years(ref, 1)
    n = 50_000
    seeds = np.random.default_rng(12345).integers(0, 2**63, n).astype(np.uint64)
    cfg = hh.SimulationConfig(n, steps=100, seeds=seeds, variance_reduction=hh.Antithetic())
    prob = hh.PricingProblem(hh.VanillaOption(100.0, expiry, hh.American(), hh.Put(), hh.Spot()),
                             hh.BlackScholesInputs(ref, 0.05, 100.0, 0.2))
    sol = hh.solve(prob, hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg, 5), path_state="spot")
    T = hh.yearfrac(ref, expiry)
    assert sol.price == pytest.approx(analytic.crr_price(100, 100, 0.05, 0.2, T, 1000, cp=-1.0), rel=0.02)


# ---- 6. Heston sanity checks -------------------------------------------------------------------------------------

def test_heston_american_against_european_on_the_same_draws(hhlib):
    """2·10^5 trajectories x 50 dates of H252, T = 1, degree 3; European prices by hh_mc_solve on the same seeds.

    Put: the American price is at least the European one; LSM is biased low only through its sub-optimal policy
    (which can do no worse than never exercising early: the European payoff) and high only through the in-sample
    foresight of the regression, O((degree + 1)/n) of the price — so American >= European - 3 combined standard
    errors.

    Call, r >= 0, no dividends: early exercise is never optimal, so the true American price IS the European one.
    LSM's estimate differs by the two biases above: the foresight bias (degree + 1 = 4 fitted coefficients per
    date over >= 10^4 in-the-money paths: < 10^-3 relative) and the loss of a policy that exercises where the
    fitted continuation falls below S - K although the true one is >= S - K·D^(N-t) — at most the interest on the
    strike over the remaining dates, K(1 - e^{-r(T-t)}) <= 3 % of K, on the few paths the fit misjudges.  We allow
    1 % of the European price for both together (Longstaff & Schwartz 2001, table 1, report LSM errors within a few
    tenths of a percent of the price at comparable sizes), plus 3 combined standard errors."""
    n, N, T, degree = 200_000, 50, 1.0, 3
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    D = math.exp(-H252["r"] * T / N)
    for cp in (-1.0, 1.0):
        m = model(HES, H252, T=T, strike=100.0, cp=cp)
        c = o.make_config(HES, EM, n, N, seeds=seeds)
        am, _, _, _ = lsm_euler(hhlib, m, c, SPOT, degree, D, want_grid=False)
        eu = _ffi.hh_result()
        hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(eu), None))
        se = math.hypot(am.std_error, eu.std_error)
        if cp < 0:
            assert am.price >= eu.price - 3 * se
        else:
            assert abs(am.price - eu.price) <= 3 * se + 0.01 * eu.price


# ---- 7. host mirror ----------------------------------------------------------------------------------------------

def _heston_problem(style=None):
    ref = hh.Date(2021, 1, 1)
    mkt = hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    return hh.PricingProblem(hh.VanillaOption(100.0, hh.Date(2022, 1, 1), style or hh.American(), hh.Put(), hh.Spot()),
                             mkt)


def test_host_mirror(hhlib):
    n, steps = 20_000, 25
    cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64),
                              variance_reduction=hh.Antithetic())
    prob = _heston_problem()
    method = hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, 4)
    sol = hh.solve(prob, method, spot_paths=True, path_state="spot")
    assert isinstance(sol, hh.LSMSolution) and sol.spot_paths.shape == (steps + 1, 2 * n)
    paths = hh.simulate_euler_paths(prob, method.mc_method)
    np.testing.assert_array_equal(paths.spot, sol.spot_paths)
    assert paths.variance.shape == (steps + 1, 2 * n) and paths.times[-1] == 1.0
    # the European solve of the same MonteCarlo: its terminal samples are the last row
    eu = hh.solve(_heston_problem(hh.European()), method.mc_method)
    assert sol.price >= eu.price - 3 * math.hypot(sol.std_error, eu.std_error)
    logs = hh.simulate_euler_paths(prob, method.mc_method, path_state="log")
    np.testing.assert_allclose(np.exp(logs.spot), paths.spot, rtol=1e-14)
    assert logs.variance is not None
    np.testing.assert_array_equal(logs.variance, paths.variance)
    # the default is today's: Euler is not an LSM path source without a named path state
    with pytest.raises(hh.MethodError):
        hh.solve(prob, method)
    with pytest.raises(ValueError):
        hh.solve(prob, method, path_state="exp")
    # "log" has no meaning on an exact source; "spot" is what it does anyway
    exact = hh.LSM(hh.HestonDynamics(), hh.HestonBroadieKaya(), hh.SimulationConfig(1000, steps=4), 3)
    with pytest.raises(hh.MethodError):
        hh.solve(prob, exact, path_state="log")
    a, b = hh.solve(prob, exact, path_state="spot"), hh.solve(prob, exact)
    assert a.price == b.price
    # duals stay refused
    dual_prob = hh.PricingProblem(prob.payoff, hh.HestonInputs(hh.Date(2021, 1, 1), 0.03, hh.Dual(100.0, (1.0,)),
                                                               0.04, 2.0, 0.04, 0.3, -0.7))
    with pytest.raises(hh.MethodError):
        hh.solve(dual_prob, method, path_state="spot")
    # lognormal paths carry no variance
    bs = hh.PricingProblem(prob.payoff, hh.BlackScholesInputs(hh.Date(2021, 1, 1), 0.03, 100.0, 0.2))
    gp = hh.simulate_euler_paths(bs, hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg))
    assert gp.variance is None and gp.spot.shape == (steps + 1, 2 * n)


# ---- 8. argument errors ------------------------------------------------------------------------------------------

def test_grid_argument_errors(hhlib):
    m = model(HES, H252, T=1.0)
    seeds = np.arange(1, 11, dtype=np.uint64)
    spot, var = np.zeros((3, 10)), np.zeros((3, 10))

    def call(c, state=SPOT, mm=m, v=None):
        return hhlib.lib.hh_euler_grid(hhlib.handle, C.byref(mm), C.byref(c), state, spot.ctypes.data,
                                       v, 0, None)

    def lsm(c, state=SPOT):
        res = _ffi.hh_lsm_result()
        return hhlib.lib.hh_lsm_solve_euler(hhlib.handle, C.byref(m), C.byref(c), state, 3, 0.99, C.byref(res),
                                            None, None, None)

    ok = o.make_config(HES, EM, 10, 2, seeds=seeds)
    assert call(ok) == _ffi.HH_OK and call(ok, v=var.ctypes.data) == _ffi.HH_OK
    assert np.all(var[0] == m.V0)
    assert call(ok, state=2) == _ffi.HH_ERR_INVALID and lsm(ok, state=-1) == _ffi.HH_ERR_INVALID
    # other strategies, REPLAY, duals: not this source
    for c in (o.make_config(HES, _ffi.HH_BROADIE_KAYA, 10, 2, seeds=seeds),
              o.make_config(GBM, _ffi.HH_EXACT_LAW, 10, 2, seeds=seeds),
              o.make_config(HES, EM, 10, 2, noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4096)),
              o.make_config(HES, EM, 10, 2, seeds=seeds, n_partials=1)):
        assert call(c) == _ffi.HH_ERR_UNSUPPORTED and lsm(c) == _ffi.HH_ERR_UNSUPPORTED
    # variance rows belong to Heston
    g = o.make_config(GBM, EM, 10, 2, seeds=seeds)
    assert call(g) == _ffi.HH_OK
    assert call(g, v=var.ctypes.data) == _ffi.HH_ERR_UNSUPPORTED
    # shapes and seeds
    assert call(o.make_config(HES, EM, 10, 0, seeds=seeds)) == _ffi.HH_ERR_INVALID
    assert call(o.make_config(HES, EM, 0, 2, seeds=seeds)) == _ffi.HH_ERR_INVALID
    assert call(o.make_config(HES, EM, 10, 70_000, seeds=seeds)) == _ffi.HH_ERR_INVALID
    c = o.make_config(HES, EM, 10, 2, seeds=seeds[:4])
    assert call(c) == _ffi.HH_ERR_INVALID and lsm(c) == _ffi.HH_ERR_INVALID  # one seed per trajectory
    assert b"seeds" in hhlib.lib.hh_last_error(hhlib.handle)
    c = o.make_config(HES, EM, 10, 2)
    assert call(c) == _ffi.HH_ERR_INVALID  # no seeds at all
    assert call(ok, mm=model(HES, {**H252, "rho": 1.5}, T=1.0)) == _ffi.HH_ERR_INVALID
    assert call(ok, mm=model(HES, H252, T=0.0)) == _ffi.HH_ERR_INVALID
    # hh_lsm_solve keeps refusing Euler
    res = _ffi.hh_lsm_result()
    assert hhlib.lib.hh_lsm_solve(hhlib.handle, C.byref(m), C.byref(ok), 3, 0.99, C.byref(res), None, None,
                                  None) == _ffi.HH_ERR_UNSUPPORTED
    assert call(ok) == _ffi.HH_OK  # and the context is fine


def test_path_offset_is_not_read(hhlib):
    """As in every Euler solve, trajectory i takes seeds[i]: an offset changes neither the grid nor the solve."""
    n, N = 1000, 12
    m = model(HES, H252, T=1.0)
    seeds = seeds_for(n, 3)
    c0 = o.make_config(HES, EM, n, N, antithetic=1, seeds=seeds)
    c5 = o.make_config(HES, EM, n, N, antithetic=1, seeds=seeds, path_offset=5)
    np.testing.assert_array_equal(euler_grid(hhlib, m, c5, SPOT)[0], euler_grid(hhlib, m, c0, SPOT)[0])
    a = lsm_euler(hhlib, m, c0, SPOT, 3, 0.999, want_grid=False)
    b = lsm_euler(hhlib, m, c5, SPOT, 3, 0.999, want_grid=False)
    assert a[0].price == b[0].price
    np.testing.assert_array_equal(a[1], b[1])
