"""State rows (log spot, variance) of the stochastic-volatility walks (hh_mc_path_states) and LSM on (S, V) on them
(hh_lsm_solve_path_states; the descriptor kind HH_LSM_STATES_LOG_SPOT_VARIANCE of hh_lsm_solve_states): what the host and the
device tests share.

  * the sources whose walk holds a variance — path_grid_cases' Heston Euler (both em_split forms), QE and Bates members, on
    that module's models, seeds and shapes — each with its statistics call, here WITH var_T where the entry point has one;
  * the two entry points as numpy calls;
  * the new kind's column rule restated: pay = cp·(exp(x_0) − K), regressors v_0 = exp(x_0), v_1 = x_1 as stored;
  * assets_lsm_cases.numpy_lsm's scheme with those regressors (np.linalg.lstsq per date on the standardised monomials);
  * the Heston cases of the price tests and the constructed grid on which the variance alone decides.
"""
import ctypes as C
import math

import numpy as np

from hedgehog_jl_amd import _ffi
from tests import assets_lsm_cases as A
from tests import path_grid_cases as pg

KIND = 1  # HH_LSM_STATES_LOG_SPOT_VARIANCE, as the header numbers it
STEPS, DIVISORS, SIZES, BIG = pg.STEPS, pg.DIVISORS, (1, 63, 64, 65, 257), 513


def state_sources():
    """the walks that hold a variance: Heston Euler in both em_split forms, QE and Bates with and without the correction"""
    return [pg.euler("euler-heston", pg.HES, pg.H252), pg.euler("euler-heston-unsplit", pg.HES, pg.H252, split=0),
            pg.qe(0), pg.qe(1), pg.bates(0), pg.bates(1)]


def no_variance_sources():
    """the walks that hold none: the Euler source under lognormal dynamics, Merton, local volatility, Variance Gamma"""
    return [pg.euler(), pg.merton(), pg.localvol(1, 64), pg.vg()]


def path_states(ctx, src, m, c, every):
    """rows[date][state][column] of hh_mc_path_states: state 0 the log spot, state 1 the variance"""
    rows = np.full((c.n_steps // every + 1, 2, pg.n_total(c)), np.nan)
    assert rows.size == ctx.lib.hh_assets_rows_elems(c.n_paths, c.n_steps // every, 2, c.antithetic)
    res, source = _ffi.hh_result(), src.source()
    ctx.check(ctx.lib.hh_mc_path_states(ctx.handle, C.byref(source), C.byref(m), C.byref(c), every, rows.ctypes.data, 0,
                                        C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return rows


def lsm_states(ctx, src, m, c, every, degree, D, want_rows=False, want_coef=False):
    """hh_lsm_solve_path_states -> (result, stop_time, stop_value, coef or None, rows or None)"""
    ntot, n_dates = pg.n_total(c), c.n_steps // every
    tau, val = np.zeros(ntot, dtype=np.int32), np.zeros(ntot)
    coef = np.full((n_dates, len(A.basis(2, degree))), np.nan) if want_coef else None
    rows = np.full((n_dates + 1, 2, ntot), np.nan) if want_rows else None
    res, source = _ffi.hh_lsm_result(), src.source()
    ctx.check(ctx.lib.hh_lsm_solve_path_states(ctx.handle, C.byref(source), C.byref(m), C.byref(c), every, degree, D,
                                               C.byref(res), tau.ctypes.data, val.ctypes.data,
                                               coef.ctypes.data if want_coef else None, rows.ctypes.data if want_rows else None))
    return res, tau, val, coef, rows


def stats_with_var_T(ctx, src, m, c, every, start=0):
    """(the five statistics, var_T or None) of the source's path_stats call on the same trajectories"""
    stats = np.full((_ffi.HH_PATH_STATS, pg.n_total(c)), np.nan)
    if src.kind == _ffi.HH_SOURCE_EULER:
        ctx.check(ctx.lib.hh_mc_path_stats(ctx.handle, C.byref(m), C.byref(c), every, start, stats.ctypes.data, 0, None))
        return stats, None
    var_T = np.full(pg.n_total(c), np.nan)
    s = src.structs
    if src.kind == _ffi.HH_SOURCE_QE:
        ctx.check(ctx.lib.hh_mc_path_stats_qe(ctx.handle, C.byref(m), C.byref(s["qe"]), C.byref(c), every, start,
                                              stats.ctypes.data, 0, var_T.ctypes.data, None))
    else:
        ctx.check(ctx.lib.hh_mc_path_stats_bates(ctx.handle, C.byref(m), C.byref(s["qe"]), C.byref(s["jump"]), C.byref(c), every,
                                                 start, stats.ctypes.data, 0, var_T.ctypes.data, None))
    return stats, var_T


# ---- the new kind's column rule and the induction on it, in numpy ----------------------------------------------------------

def desc(cp, K, n_states=2, kind=KIND):
    d = _ffi.hh_lsm_states()
    d.kind, d.n_states, d.cp, d.strike = kind, n_states, cp, K
    d.index_kind = -7          # not read under this kind …
    for i in range(_ffi.HH_MAX_ASSETS):
        d.weights[i] = float("nan")  # … nor are the weights
    return d


def regressors(row):
    """v[i][column] of a date's states row[state][column]: the spot and the variance as stored"""
    return np.stack([np.exp(row[0]), row[1]])


def pay_of(row, cp, K):
    return cp * (np.exp(row[0]) - K)


def numpy_lsm(rows, cp, K, degree, D):
    """assets_lsm_cases.numpy_lsm with the regressors above -> (price, tau, val, per-date (pay, cont, in-the-money mask,
    condition number of the scaled Gram matrix, max |y|))"""
    n_dates = rows.shape[0] - 1
    expo = A.basis(2, degree)
    tau = np.full(rows.shape[2], n_dates)
    val = np.maximum(pay_of(rows[n_dates], cp, K), 0.0)
    dates = {}
    for t in range(n_dates - 1, 0, -1):
        pay = pay_of(rows[t], cp, K)
        itm = pay > 0.0
        if not itm.any():
            continue
        v = regressors(rows[t])[:, itm]
        mu, sd = v.mean(axis=1), v.std(axis=1)
        sd[sd == 0] = 1.0
        P = A.phi((v - mu[:, None]) / sd[:, None], expo)
        y = D ** (tau[itm] - t) * val[itm]
        c = np.linalg.lstsq(P.T, y, rcond=None)[0]
        cont = c @ P
        G = P @ P.T
        s = np.sqrt(np.diag(G))
        s[s == 0] = 1.0
        dates[t] = (pay[itm], cont, itm, float(np.linalg.cond(G / np.outer(s, s))), float(np.max(np.abs(y))))
        ex = pay[itm] > cont
        idx = np.nonzero(itm)[0][ex]
        tau[idx], val[idx] = t, pay[itm][ex]
    return float(np.mean(D ** tau * val)), tau, val, dates


# ---- the price cases: an at-the-money put at K = S0 = 100, r = 0.05 ----------------------------------------------------------

R, STRIKE = 0.05, 100.0
PRICE_N, PRICE_STEPS, PRICE_EVERY, DEGREE = 200_000, 48, 4, 3   # 12 exercise dates
HESTON = {
    "wild": dict(S0=100.0, V0=0.16, kappa=0.5, theta=0.16, sigma=1.5, rho=0.0, r_drift=R, T=2.0),
    "mid": dict(S0=100.0, V0=0.09, kappa=1.0, theta=0.09, sigma=1.0, rho=-0.3, r_drift=R, T=1.0),
}
LAM = 0.8  # jumps per year of the Bates member (path_grid_cases' price source)


def price_source(which, name):
    """the martingale correction where ρ < 0 (at ρ = 0 its admission test, A <= 0, sits on A = 0)"""
    case = HESTON[name]
    mart = int(case["rho"] < 0.0)
    if which == "euler":
        return pg.euler("euler-" + name, pg.HES, pg._case_params(case))
    if which == "qe":
        return pg.qe(mart, case, "qe-" + name)
    return pg.bates(mart, LAM, case, "bates-" + name)


def price_case(src, name, n=PRICE_N, steps=PRICE_STEPS):
    m = src.model(T=HESTON[name]["T"], strike=STRIKE, cp=-1.0)
    return m, src.config(n, steps, 0, seeds=np.arange(1, n + 1, dtype=np.uint64))


def date_discount(m, steps, every):
    return math.exp(-m.r_drift * m.T * every / steps)


# ---- a grid on which the variance alone decides ------------------------------------------------------------------------------

def variance_decides_grid(n=513):
    """Two dates, a put at K = 100, D = 1.  Date 1: S = 90 in every column, v_i = 0.08·(i + ¼)/n — evenly spread over
    [0, 0.08], the nearest to 0.04 at a distance of 0.02/n.  Date 2: S_2 = 90 + 200·(v_i − 0.04), so the continuation value is
    10 − 200·(v − 0.04), linear in v, against an exercise value of 10: exercise exactly where v > 0.04."""
    v = 0.08 * (np.arange(n) + 0.25) / n
    rows = np.empty((3, 2, n))
    rows[0, 0], rows[0, 1] = math.log(100.0), 0.04
    rows[1, 0], rows[1, 1] = math.log(90.0), v
    rows[2, 0], rows[2, 1] = np.log(90.0 + 200.0 * (v - 0.04)), v
    return rows, v
