"""Dual bounds for American exercise on the device: the policy as an array (hh_lsm_fit_states, hh_lsm_fit_path_states), its
value run forward (hh_lsm_policy_value, hh_lsm_policy_value_path) and the Andersen–Broadie upper bound by nested simulation
(hh_lsm_upper_bound).  Restatements: tests/bounds_cases.py.

1 the policy is the induction's: coefficients and prices bit for bit, μ and isd against the header's formulas;
2 run forward on the rows it was fitted on, a policy stops every column where the induction stopped it;
3 hand-made policies against numpy on downloaded rows;
4 nested continuation values against the Black–Scholes put where the Euler walk is the exact lognormal law;
5 the outer recursion against numpy on the downloaded rows and continuation values;
6 a bracket around a Bermudan binomial tree;  7 the bracket under stochastic volatility;  8 every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from tests import assets_lsm_cases as A
from tests import bounds_cases as bc
from tests import path_grid_cases as pg
from tests import path_states_cases as ps

pytestmark = pytest.mark.gpu

HESTON = pg.euler("euler-heston", pg.HES, pg.H252)
LOGN = bc.lognormal_source()
# σ = 0 and V0 = θ = 2^-4: every trajectory keeps V0, and the sums of the constant regressor are exact — its variance is 0
CONSTV = pg.euler("euler-constant-variance", pg.HES, dict(pg.H252, V0=0.0625, theta=0.0625, sigma=0.0))
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def seeds(first, n):
    return np.arange(first, first + n, dtype=np.uint64)


def on_device(rows):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return dev


def fit_states(ctx, dev, shape, desc, degree, D):
    """hh_lsm_fit_states on device rows -> (result, tau, val, policy)"""
    n_dates, m, ntot = shape[0] - 1, shape[1], shape[2]
    tau, val, policy = np.zeros(ntot, dtype=np.int32), np.zeros(ntot), np.full(bc.policy_shape(n_dates, degree, m), np.nan)
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_fit_states(ctx.handle, C.byref(desc), dev.data_ptr(), ntot, n_dates, degree, D, C.byref(res),
                                        tau.ctypes.data, val.ctypes.data, policy.ctypes.data))
    return res, tau, val, policy


def value_states(ctx, dev, shape, desc, policy, degree, D):
    """hh_lsm_policy_value on device rows -> (result, tau, val)"""
    n_dates, ntot = shape[0] - 1, shape[2]
    tau, val = np.full(ntot, -1, dtype=np.int32), np.full(ntot, np.nan)
    res = _ffi.hh_lsm_result()
    policy = np.ascontiguousarray(policy)
    ctx.check(ctx.lib.hh_lsm_policy_value(ctx.handle, C.byref(desc), policy.ctypes.data, degree, dev.data_ptr(), ntot, n_dates, D,
                                          C.byref(res), tau.ctypes.data, val.ctypes.data))
    return res, tau, val


# ---- 1. the policy is the induction's --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [2, 3])
def test_the_policy_is_the_inductions(hhlib, degree):
    """μ and isd against a float64 numpy restatement of the header's formulas to 1e-12 relative: the device adds in its own tree,
    numpy pairwise, so this is a bound on the conditioning of Σv, Σv² over <= 4096 columns (κ(Σ) = 1: all terms positive for the
    spot; the variance Σv²/n − μ² loses a factor μ²/var <= 10^3 of it), not a statement about bits."""
    n, steps, every = 4096, 24, 4
    m, c = HESTON.model(strike=100.0, cp=-1.0), HESTON.config(n, steps)
    D = ps.date_discount(m, steps, every)
    res0, tau0, val0, coef0, rows = ps.lsm_states(hhlib, HESTON, m, c, every, degree, D, want_rows=True, want_coef=True)
    res, policy = bc.fit_path(hhlib, HESTON, m, c, every, degree, D)
    n_dates = steps // every
    mu, isd, coef = bc.parts(policy)
    assert np.array_equal(coef[:n_dates], coef0) and np.all(coef[n_dates] == 0.0) and np.any(coef0 != 0.0)
    assert (res.price, res.std_error, res.rows_regressed, res.rows_skipped) == (res0.price, res0.std_error, res0.rows_regressed,
                                                                                res0.rows_skipped)
    for t in (0, n_dates):
        assert np.all(mu[t] == 0.0) and np.all(isd[t] == 1.0)
    for t in range(1, n_dates):
        cnt, mu_np, isd_np = bc.row_statistics(rows[t], -1.0, 100.0)
        assert cnt > 100
        np.testing.assert_allclose(mu[t], mu_np, rtol=1e-12)
        np.testing.assert_allclose(isd[t], isd_np, rtol=1e-12)


# ---- 2. forward valuation reproduces the induction in sample --------------------------------------------------------------------

def _walk_rows(ctx, src, n, steps, every):
    m, c = src.model(strike=100.0, cp=-1.0), src.config(n, steps)
    return ps.path_states(ctx, src, m, c, every), ps.date_discount(m, steps, every)


def _no_money_rows(n):
    """four dates about the money; on date 2 every column is far above the strike of a put: no column in the money"""
    rng = np.random.default_rng(n)
    rows = np.empty((5, 2, n))
    rows[0, 0], rows[0, 1] = math.log(100.0), 0.09
    for t in range(1, 5):
        rows[t, 0] = rows[t - 1, 0] + 0.1 * rng.standard_normal(n)
        rows[t, 1] = 0.09 + 0.05 * rng.standard_normal(n)
    rows[2, 0] += 2.0
    return rows


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("n", [65, 513, 4096])
@pytest.mark.parametrize("case", ["heston", "constant-variance", "no-column-in-the-money"])
def test_forward_valuation_reproduces_the_induction_in_sample(hhlib, case, n, degree):
    """LSM stops a column at the first date its fitted rule fires: the rule run forward on the fitted rows must stop every
    column where the induction did, with the same value, and give the same price bits.  constant-variance: σ = 0 and V0 = θ,
    the variance regressor is constant, its monomials are dropped pivots.  65 and 513: the tails of a wave and a workgroup."""
    if case == "no-column-in-the-money":
        rows, D = cached((case, n), lambda: _no_money_rows(n)), 0.99
    else:
        src = HESTON if case == "heston" else CONSTV
        rows, D = cached((case, n), lambda: _walk_rows(hhlib, src, n, 24, 4))
    desc = ps.desc(-1.0, 100.0)
    dev = on_device(rows)
    res0, tau0, val0, policy = fit_states(hhlib, dev, rows.shape, desc, degree, D)
    res, tau, val = value_states(hhlib, dev, rows.shape, desc, policy, degree, D)
    assert np.array_equal(tau, tau0) and np.array_equal(val, val0)
    assert (res.price, res.std_error, res.n_paths_total) == (res0.price, res0.std_error, n)
    assert np.all(np.isfinite(policy))
    mu, isd, coef = bc.parts(policy)
    if case == "no-column-in-the-money":
        assert res0.rows_skipped == 1 and np.all(coef[2] == 0.0) and np.all(mu[2] == 0.0) and np.all(isd[2] == 1.0)
        assert not np.any(tau == 2)
    if case == "constant-variance":
        with_v = [j for j, e in enumerate(A.basis(2, degree)) if e[1] > 0]
        assert np.all(coef[:, with_v] == 0.0) and np.all(isd[1:-1, 1] == 1.0) and np.any(coef != 0.0)
    if n == 4096:
        assert 1 < len(np.unique(tau))  # the policy does exercise early somewhere


# ---- 3. hand-made policies -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [1, 3])
def test_hand_made_policies(hhlib, degree):
    """c_0 = 1e300: every column stops at expiry.  All zeros: at the first date in the money.  Stopping dates against numpy
    exactly; the stopped value is cp·(exp(x) − K) with the device's own exp (<= 1 ulp), so it is held to one spacing of the spot."""
    rows, D = cached(("heston", 513), lambda: _walk_rows(hhlib, HESTON, 513, 24, 4))
    n_dates, desc, dev = rows.shape[0] - 1, ps.desc(-1.0, 100.0), on_device(rows)
    spots = np.exp(rows[:, 0])
    for policy in (bc.never_policy(n_dates, degree), bc.zero_policy(n_dates, degree), bc.blank_policy(n_dates, degree)):
        res, tau, val = value_states(hhlib, dev, rows.shape, desc, policy, degree, D)
        tau_np, val_np = bc.forward_value(rows, policy, -1.0, 100.0, degree)
        assert np.array_equal(tau, tau_np)
        assert np.all(np.abs(val - val_np) <= np.spacing(spots[tau_np, np.arange(513)]))
        assert res.price == pytest.approx(float(np.mean(D ** tau_np * val_np)), rel=1e-13)
    res, tau, val = value_states(hhlib, dev, rows.shape, desc, bc.never_policy(n_dates, degree), degree, D)
    assert np.all(tau == n_dates)
    res, tau, val = value_states(hhlib, dev, rows.shape, desc, bc.zero_policy(n_dates, degree), degree, D)
    pays = np.stack([ps.pay_of(rows[t], -1.0, 100.0) for t in range(n_dates + 1)])
    first = np.array([next((t for t in range(1, n_dates) if pays[t, i] > 0.0), n_dates) for i in range(513)])
    assert np.array_equal(tau, first) and tau.min() == 1


# ---- 4. nested continuation values against a closed form ---------------------------------------------------------------------

def _lognormal_outer(n=512):
    m = LOGN.model(T=bc.LOGN_T, strike=bc.LOGN_K, cp=-1.0)
    return m, LOGN.config(n, bc.LOGN_STEPS, seeds=seeds(7_000_001, n))


def _never_bound(ctx, inner_seed=11):
    m, c = _lognormal_outer()
    D = ps.date_discount(m, bc.LOGN_STEPS, bc.LOGN_EVERY)
    return bc.upper_bound(ctx, m, c, bc.LOGN_EVERY, bc.never_policy(12, 2), 2, D, 256, inner_seed)


def test_nested_continuation_values_against_black_scholes(hhlib):
    """σ = 0 and V0 = θ = 0.04 (the Euler validation admits σ = 0: it checks finiteness): the walk is the exact lognormal law at
    vol 0.2, and under the never-exercise policy Ĉ[t][i] estimates the Black–Scholes put on (exp(x_{t,i}), T − t·T/12).

    THE BARS.  The per-pair bar one would write first — Ĉ within 5 of its OWN cont_se for all 6144 pairs, the scores' mean within
    ±0.1 and variance in 0.8 .. 1.25 — is a condition on a unit normal sample, and these scores are not one: a float64
    numpy restatement of this experiment (exact lognormal draws, numpy's generator, 20 runs) leaves it.  Deep out of the money
    all 256 inner payoffs are 0, cont_se = 0 and the score is −∞; and the studentised mean of 256 skewed payoffs has tails to
    5.8 – 7.0 in 4 of 20 runs even where 10 – 20 % of the payoffs are positive.  What the restatement does satisfy, with room, in
    20 of 20 runs, and what is asserted here with the same numbers: on the pairs whose payoff is positive with probability
    N(−d2) >= 0.2 (about 4700 of the 6144), the score against the EXACT standard error sqrt(Var y / 256) (closed form,
    bounds_cases.put_moments) has |z| <= 5 for every pair (restatement: <= 4.44), mean within ±0.1 (±0.02) and variance in
    0.8 .. 1.25 (0.97 .. 1.02); the studentised score there has mean within ±0.1 and variance in 0.8 .. 1.25 as well
    (−0.03 .. −0.06, 1.01 .. 1.05) and its maximum is printed; cont_se is 0.5 .. 1.6 of the exact standard error (0.60 .. 1.44).
    On the other pairs the deviations are added up: Σ(Ĉ − BS)/sqrt(ΣVar y/256) within ±5 (±1.6), a sum of >= 1000 independent
    terms."""
    m, c = _lognormal_outer()
    res, cont, se, pmax = cached("never-bound", lambda: _never_bound(hhlib))
    rows = cached("lognormal-outer-rows", lambda: ps.path_states(hhlib, LOGN, m, c, bc.LOGN_EVERY))
    assert np.all(rows[:, 1] == 0.04) and (res.n_outer, res.n_inner) == (512, 256) and res.nested_ms > 0.0
    z_exact, z_own, ratio, dev, var = [], [], [], [], []
    for t in range(12):
        mean, v, p = bc.put_moments(np.exp(rows[t, 0]), bc.LOGN_K, bc.LOGN_R, bc.LOGN_VOL, bc.LOGN_T * (1.0 - t / 12.0))
        k = p >= 0.2
        z_exact.append((cont[t, k] - mean[k]) / np.sqrt(v[k] / 256.0))
        z_own.append((cont[t, k] - mean[k]) / se[t, k])
        ratio.append(se[t, k] / np.sqrt(v[k] / 256.0))
        dev.append(cont[t, ~k] - mean[~k])
        var.append(v[~k] / 256.0)
    z_exact, z_own, ratio, dev, var = map(np.concatenate, (z_exact, z_own, ratio, dev, var))
    rest = float(dev.sum() / math.sqrt(var.sum()))
    print(f"\n{z_exact.size} pairs with N(-d2) >= 0.2: exact-se z max {np.abs(z_exact).max():.2f} mean {z_exact.mean():+.3f} var "
          f"{z_exact.var():.3f}; own-se z max {np.abs(z_own).max():.2f} mean {z_own.mean():+.3f} var {z_own.var():.3f}; cont_se / exact "
          f"{ratio.min():.2f} .. {ratio.max():.2f}; the other {dev.size} pairs added up: {rest:+.2f}")
    assert z_exact.size > 4000 and dev.size > 1000
    assert np.abs(z_exact).max() <= 5.0 and abs(z_exact.mean()) <= 0.1 and 0.8 <= z_exact.var() <= 1.25
    assert abs(z_own.mean()) <= 0.1 and 0.8 <= z_own.var() <= 1.25
    assert 0.5 <= ratio.min() and ratio.max() <= 1.6
    assert abs(rest) <= 5.0
    assert np.all(cont >= 0.0) and np.all(se >= 0.0) and np.all((se > 0.0) | (cont == 0.0))
    # the same call gives the same bits; another inner_seed other values
    res2, cont2, se2, pmax2 = _never_bound(hhlib)
    assert np.array_equal(cont, cont2) and np.array_equal(se, se2) and np.array_equal(pmax, pmax2)
    assert (res2.upper, res2.upper_se) == (res.upper, res.upper_se)
    res3, cont3, _, _ = _never_bound(hhlib, inner_seed=12)
    assert np.mean(cont3 != cont) > 0.9 and res3.upper != res.upper


# ---- 5. the outer pass exactly ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["never", "fitted"])
def test_the_outer_pass_against_numpy(hhlib, which):
    m, c = _lognormal_outer()
    D = ps.date_discount(m, bc.LOGN_STEPS, bc.LOGN_EVERY)
    rows = cached("lognormal-outer-rows", lambda: ps.path_states(hhlib, LOGN, m, c, bc.LOGN_EVERY))
    if which == "never":
        policy, degree = bc.never_policy(12, 2), 2
        res, cont, se, pmax = cached("never-bound", lambda: _never_bound(hhlib))
    else:
        degree = 3
        fit_c = LOGN.config(20_000, bc.LOGN_STEPS, seeds=seeds(1, 20_000))
        _, policy = bc.fit_path(hhlib, LOGN, m, fit_c, bc.LOGN_EVERY, degree, D)
        res, cont, se, pmax = bc.upper_bound(hhlib, m, c, bc.LOGN_EVERY, policy, degree, D, 64, 5)
    want = bc.dual_outer(rows, cont, policy, -1.0, bc.LOGN_K, degree, D)
    np.testing.assert_allclose(pmax, want, rtol=1e-12)
    assert res.upper == pytest.approx(float(want.mean()), rel=1e-12)
    assert res.upper_se == pytest.approx(float(want.std(ddof=1) / math.sqrt(want.size)), rel=1e-9)
    assert pmax.min() > 0.0


# ---- 6. a bracket around a known price -------------------------------------------------------------------------------------------

def _bracket(ctx, src, m, steps, every, degree, n_fit, n_outer, n_inner, label):
    """fit on seeds 1 .., fresh on the next n_fit, outer on the n_outer after those -> the figures, printed"""
    D = ps.date_discount(m, steps, every)
    n_dates = steps // every
    fit, policy = bc.fit_path(ctx, src, m, src.config(n_fit, steps, seeds=seeds(1, n_fit)), every, degree, D)
    low = bc.value_path(ctx, src, m, src.config(n_fit, steps, seeds=seeds(n_fit + 1, n_fit)), every, policy, degree, D)
    outer = src.config(n_outer, steps, seeds=seeds(2 * n_fit + 1, n_outer))
    up, *_ = bc.upper_bound(ctx, m, outer, every, policy, degree, D, n_inner, 2024, want=False)
    never, *_ = bc.upper_bound(ctx, m, outer, every, bc.never_policy(n_dates, degree), degree, D, n_inner, 2024, want=False)
    print(f"\n{label}: in sample {fit.price:.4f} ± {fit.std_error:.4f}; lower {low.price:.4f} ± {low.std_error:.4f}; upper "
          f"{up.upper:.4f} ± {up.upper_se:.4f}; gap {up.upper - low.price:.4f} ± {math.hypot(up.upper_se, low.std_error):.4f}; "
          f"never-exercise upper {never.upper:.4f} ± {never.upper_se:.4f}; nested {up.nested_ms:.1f} ms, outer {up.outer_ms:.3f} ms")
    return fit, low, up, never


def test_a_bracket_around_the_bermudan_tree(hhlib):
    """The lognormal case as a Bermudan put on 12 dates; the reference is a binomial tree of 1200 steps with exercise on every
    100th (2400 steps move it by 1.4e-4, far inside the Monte Carlo standard errors of about 0.01)."""
    tree = bc.bermudan_tree(100.0, bc.LOGN_K, bc.LOGN_R, bc.LOGN_VOL, bc.LOGN_T, 1200, 100)
    m = LOGN.model(T=bc.LOGN_T, strike=bc.LOGN_K, cp=-1.0)
    fit, low, up, never = _bracket(hhlib, LOGN, m, bc.LOGN_STEPS, bc.LOGN_EVERY, 3, 200_000, 4096, 256, f"lognormal, tree {tree:.4f}")
    assert low.price - 4.0 * low.std_error <= tree <= up.upper + 4.0 * up.upper_se
    assert up.upper < never.upper - 4.0 * math.hypot(up.upper_se, never.upper_se)  # the bound is informative


# ---- 7. stochastic volatility ----------------------------------------------------------------------------------------------------

def test_the_bracket_under_stochastic_volatility(hhlib):
    """DESIGN §5.22's case: κ 0.5, θ = V0 = 0.16, σ 1.5, ρ 0, T 2, 48 steps, 12 dates, degree 3"""
    src = ps.price_source("euler", "wild")
    m = src.model(T=bc.SV["T"], strike=ps.STRIKE, cp=-1.0)
    fit, low, up, never = _bracket(hhlib, src, m, ps.PRICE_STEPS, ps.PRICE_EVERY, ps.DEGREE, ps.PRICE_N, 4096, 256, "Heston §5.22")
    assert up.upper + 4.0 * up.upper_se >= low.price - 4.0 * low.std_error
    assert low.price <= fit.price + 4.0 * math.hypot(low.std_error, fit.std_error)
    assert up.upper <= never.upper


# ---- 8. refusals: all of them before any launch ----------------------------------------------------------------------------------

def test_every_refusal_comes_back_before_a_launch(hhlib):
    import torch
    ctx, lib, h = hhlib, hhlib.lib, hhlib.handle
    INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
    n, steps, every, degree, D = 128, 12, 3, 3, 0.99
    n_dates = steps // every
    src = HESTON
    s, m, c = src.source(), src.model(strike=100.0, cp=-1.0), src.config(n, steps)
    S, M, Cc = C.byref(s), C.byref(m), C.byref(c)
    good = bc.blank_policy(n_dates, degree)
    P = good.ctypes.data
    out, bout = _ffi.hh_lsm_result(), _ffi.hh_bounds_result()
    O, BO = C.byref(out), C.byref(bout)
    desc = ps.desc(-1.0, 100.0)
    dev = torch.zeros((n_dates + 1) * 2 * n, dtype=torch.float64, device="cuda")
    R = dev.data_ptr()

    def said(rc, code, text, who):
        msg = lib.hh_last_error(h).decode()
        assert rc == code and text in msg and (who is None or who in msg), (rc, code, text, who, msg)

    def upper(M=M, Cc=Cc, every=every, P=P, degree=degree, D=D, n_inner=64, BO=BO):
        return lib.hh_lsm_upper_bound(h, M, Cc, every, P, degree, D, n_inner, 1, BO, None, None, None)

    def value_path(S=S, M=M, Cc=Cc, every=every, P=P, degree=degree, D=D, O=O):
        return lib.hh_lsm_policy_value_path(h, S, M, Cc, every, P, degree, D, O)

    def fit_path(S=S, M=M, Cc=Cc, every=every, degree=degree, D=D, O=O, P=P):
        return lib.hh_lsm_fit_path_states(h, S, M, Cc, every, degree, D, O, P)

    def value(desc=desc, P=P, degree=degree, R=R, D=D, O=O):
        return lib.hh_lsm_policy_value(h, C.byref(desc) if desc is not None else None, P, degree, R, n, n_dates, D, O, None, None)

    def fit(desc=desc, R=R, degree=degree, D=D, O=O, P=P):
        return lib.hh_lsm_fit_states(h, C.byref(desc) if desc is not None else None, R, n, n_dates, degree, D, O, None, None, P)

    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        # NULLs
        for kw in (dict(M=None), dict(Cc=None), dict(P=None), dict(BO=None)):
            said(upper(**kw), INV, "NULL argument", "hh_lsm_upper_bound")
        for call, who in ((value_path, "hh_lsm_policy_value_path"), (fit_path, "hh_lsm_fit_path_states")):
            for kw in (dict(S=None), dict(M=None), dict(Cc=None), dict(P=None), dict(O=None)):
                said(call(**kw), INV, "NULL argument", who)
        for call, who in ((value, "hh_lsm_policy_value"), (fit, "hh_lsm_fit_states")):
            for kw in (dict(desc=None), dict(P=None), dict(R=None), dict(O=None)):
                said(call(**kw), INV, "NULL argument", who)
        # n_inner
        for n_inner in (0, 1, 63, 65, 100):
            said(upper(n_inner=n_inner), INV, "n_inner", "hh_lsm_upper_bound")
        # a policy entry that is not finite
        for bad in (float("nan"), float("inf"), -float("inf")):
            policy = good.copy()
            policy[2, 5] = bad
            for call, who in ((upper, "hh_lsm_upper_bound"), (value_path, "hh_lsm_policy_value_path"), (value, "hh_lsm_policy_value")):
                said(call(P=policy.ctypes.data), INV, "policy entry 5 of date 2 is not finite", who)
        # degree, date_discount, cp and exercise_every as hh_lsm_solve_path_states checks them
        for call, who in ((upper, "hh_lsm_upper_bound"), (value_path, "hh_lsm_policy_value_path"), (fit_path, "hh_lsm_fit_path_states")):
            for bad_degree in (0, 9):
                said(call(degree=bad_degree), INV, "LSM", None)
            for bad_D in (0.0, -1.0, float("nan"), float("inf")):
                said(call(D=bad_D), INV, "LSM", None)
            said(call(M=C.byref(src.model(cp=0.5))), INV, "LSM", None)
            said(call(M=C.byref(src.model(strike=float("inf")))), INV, "strike", who)
            for bad_every in (0, 5, 24):
                said(call(every=bad_every), INV, "exercise_every", who)
            said(call(every=5, degree=0), INV, "exercise_every", who)  # the schedule first
        for call in (value, fit):
            said(call(degree=0), INV, "LSM", None)
            said(call(D=0.0), INV, "LSM", None)
            said(call(desc=ps.desc(-1.0, 100.0, kind=2)), INV, "unknown descriptor kind 2", None)
        # what hh_lsm_upper_bound does not offer
        for dyn, strat in ((pg.GBM, pg.EM), (pg.HES, pg.QE), (pg.GBM, pg.LAW), (pg.HES, _ffi.HH_BROADIE_KAYA)):
            other = _ffi.make_config(dyn, strat, n, steps, seeds=pg.seeds_for(n))
            said(upper(Cc=C.byref(other)), UNS, "needs HestonDynamics + EulerMaruyama", "hh_lsm_upper_bound")
        said(upper(Cc=C.byref(src.config(n, steps, 1))), UNS, "no antithetic outer paths", "hh_lsm_upper_bound")
        said(upper(Cc=C.byref(src.config(n, steps, noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4)))), UNS,
             "GENERATE noise, no dual partials", "hh_lsm_upper_bound")
        said(upper(Cc=C.byref(src.config(n, steps, n_partials=2))), UNS, "GENERATE noise, no dual partials", "hh_lsm_upper_bound")
        # the sources hh_mc_path_states refuses
        for other in ps.no_variance_sources():
            so, mo, co = other.source(), other.model(strike=100.0, cp=-1.0), other.config(n, steps)
            said(value_path(S=C.byref(so), M=C.byref(mo), Cc=C.byref(co)), UNS, "no variance", "hh_lsm_policy_value_path")
            said(fit_path(S=C.byref(so), M=C.byref(mo), Cc=C.byref(co)), UNS, "no variance", "hh_lsm_fit_path_states")
        assert lib.hh_lsm_policy_elems(n_dates, 2, 9) == 0 and lib.hh_lsm_policy_elems(n_dates, 9, 2) == 0
        assert ctx.read_timings() == []  # nothing was launched
        # … and the context solves: the rows and the nested kernel are a timing slot each, the forward valuation one
        assert upper() == 0 and len(ctx.read_timings()) == 2
        assert value_path() == 0 and len(ctx.read_timings()) == 2
        assert value() == 0 and len(ctx.read_timings()) == 1
    finally:
        ctx.enable_timing(False)
