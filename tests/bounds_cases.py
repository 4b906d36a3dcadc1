"""Dual bounds for American exercise (hh_lsm_fit_states, hh_lsm_policy_value, hh_lsm_upper_bound): what the host and the
device tests share.

  * the policy array's layout restated: per date μ_i, isd_i (m each), then the B coefficients; the hand-made policies;
  * the rule a policy states, in numpy: z = (v − μ)·isd, fit = Σ c_j·φ_j, exercise where pay > 0 and pay > fit;
  * the outer recursion of the dual bound, in numpy: M_t = M_{t−1} + D^t·L_t − D^{t−1}·Ĉ[t−1], max_t (D^t·pay_t⁺ − M_t);
  * the lognormal case whose continuation values have a closed form (σ = 0, V0 = θ: the Euler log walk is the exact law), the
    Black–Scholes put and a Bermudan binomial tree;
  * the entry points as numpy calls.
"""
import ctypes as C
import math

import numpy as np

from hedgehog_jl_amd import _ffi
from tests import assets_lsm_cases as A
from tests import path_grid_cases as pg
from tests import path_states_cases as ps

M = 2  # regressors of the (log S, V) rows: the spot and the variance


def n_basis(degree, m=M):
    return len(A.basis(m, degree))


def policy_shape(n_dates, degree, m=M):
    return n_dates + 1, 2 * m + n_basis(degree, m)


def blank_policy(n_dates, degree, m=M):
    """the policy of dates where no fit ran: μ = 0, isd = 1, coef = 0 — it exercises at the first date in the money"""
    p = np.zeros(policy_shape(n_dates, degree, m))
    p[:, m:2 * m] = 1.0
    return p


def never_policy(n_dates, degree, m=M):
    """c_0 = 1e300 on every date: no exercise value is above the fitted value, every column stops at expiry"""
    p = blank_policy(n_dates, degree, m)
    p[:, 2 * m] = 1e300
    return p


def zero_policy(n_dates, degree, m=M):
    """all zeros (isd too: z = 0, fit = 0): every column stops at the first date in the money"""
    return np.zeros(policy_shape(n_dates, degree, m))


def parts(policy, m=M):
    """(μ[date][i], isd[date][i], coef[date][j])"""
    return policy[:, :m], policy[:, m:2 * m], policy[:, 2 * m:]


def fitted_value(policy_row, v, degree):
    """Σ c_j·φ_j of the regressors v[i][column] under one date's policy (numpy's summation order, not the device's)"""
    m = v.shape[0]
    mu, isd, coef = policy_row[:m], policy_row[m:2 * m], policy_row[2 * m:]
    with np.errstate(over="ignore", invalid="ignore"):
        P = A.phi((v - mu[:, None]) * isd[:, None], A.basis(m, degree))
        return coef @ P


def forward_value(rows, policy, cp, K, degree):
    """the rule run forward on rows[date][state][column] of (log S, V) -> (tau, val): the first date 1 .. n_dates − 1 with
    pay > 0 and pay > fit, else expiry with max(pay, 0)"""
    n_dates, n = rows.shape[0] - 1, rows.shape[2]
    tau = np.full(n, n_dates, dtype=np.int32)
    val = np.maximum(ps.pay_of(rows[n_dates], cp, K), 0.0)
    open_ = np.ones(n, dtype=bool)
    for t in range(1, n_dates):
        pay = ps.pay_of(rows[t], cp, K)
        fit = fitted_value(policy[t], ps.regressors(rows[t]), degree)
        ex = open_ & (pay > 0.0) & (pay > fit)
        tau[ex], val[ex] = t, pay[ex]
        open_ &= ~ex
    return tau, val


def dual_outer(rows, cont, policy, cp, K, degree, D):
    """the header's recursion on downloaded rows and cont[date][column] -> pathwise_max[column]"""
    n_dates, n = rows.shape[0] - 1, rows.shape[2]
    best = np.maximum(ps.pay_of(rows[0], cp, K), 0.0)
    mart = np.zeros(n)
    for t in range(1, n_dates + 1):
        pay = ps.pay_of(rows[t], cp, K)
        payp = np.maximum(pay, 0.0)
        if t == n_dates:
            L = payp
        else:
            fit = fitted_value(policy[t], ps.regressors(rows[t]), degree)
            L = np.where((pay > 0.0) & (pay > fit), pay, cont[t])
        mart = (mart + D ** t * L) - D ** (t - 1) * cont[t - 1]
        best = np.maximum(best, D ** t * payp - mart)
    return best


def row_statistics(row, cp, K):
    """(n, μ_i, isd_i) of a date by the header's formulas on the in-the-money columns, in float64 numpy"""
    itm = ps.pay_of(row, cp, K) > 0.0
    n = int(itm.sum())
    if n == 0:
        return 0, np.zeros(M), np.ones(M)
    v = ps.regressors(row)[:, itm]
    mu = v.sum(axis=1) / n
    var = (v * v).sum(axis=1) / n - mu * mu
    return n, mu, np.where(var > 0.0, 1.0 / np.sqrt(np.where(var > 0.0, var, 1.0)), 1.0)


# ---- the lognormal case: σ = 0 and V0 = θ, so v stays at θ and log S takes exact normal increments -------------------------

LOGN = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.0, rho=0.0, r=0.05)
LOGN_VOL, LOGN_R, LOGN_K, LOGN_T, LOGN_STEPS, LOGN_EVERY = 0.2, 0.05, 100.0, 1.0, 48, 4   # 12 dates
SV = ps.HESTON["wild"]  # κ 0.5, θ = V0 = 0.16, σ 1.5, ρ 0, T 2: DESIGN §5.22's case


def lognormal_source():
    return pg.euler("euler-lognormal-in-heston", pg.HES, LOGN)


def norm_cdf(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(x, dtype=np.float64) / math.sqrt(2.0)))


def bs_put(S, K, r, vol, tau):
    """the Black–Scholes put on spots S with time tau > 0 to expiry"""
    S = np.asarray(S, dtype=np.float64)
    sd = vol * math.sqrt(tau)
    d1 = (np.log(S / K) + (r + 0.5 * vol * vol) * tau) / sd
    return K * math.exp(-r * tau) * norm_cdf(-(d1 - sd)) - S * norm_cdf(-d1)


def put_moments(S, K, r, vol, tau):
    """(mean, variance, probability of a positive payoff) of y = e^{−r·tau}·max(K − S_tau, 0) under the lognormal law from S:
    the mean is bs_put; E[(K − S)²; S < K] = K²·N(−d2) − 2·K·F·N(−d1) + F²·e^{vol²·tau}·N(−d1 − vol·√tau), F = S·e^{r·tau}"""
    S = np.asarray(S, dtype=np.float64)
    sd = vol * math.sqrt(tau)
    F = S * math.exp(r * tau)
    d2 = (np.log(F / K) - 0.5 * sd * sd) / sd
    d1 = d2 + sd
    m1 = K * norm_cdf(-d2) - F * norm_cdf(-d1)
    m2 = K * K * norm_cdf(-d2) - 2.0 * K * F * norm_cdf(-d1) + F * F * math.exp(sd * sd) * norm_cdf(-d1 - sd)
    disc = math.exp(-r * tau)
    return disc * m1, disc * disc * np.maximum(m2 - m1 * m1, 0.0), norm_cdf(-d2)


def bermudan_tree(S0, K, r, vol, T, N, every):
    """a Cox–Ross–Rubinstein put with exercise on every `every`-th of N steps (and at expiry)"""
    dt = T / N
    u = math.exp(vol * math.sqrt(dt))
    p = (math.exp(r * dt) - 1.0 / u) / (u - 1.0 / u)
    disc = math.exp(-r * dt)
    j = np.arange(N + 1)
    V = np.maximum(K - S0 * u ** (2.0 * j - N), 0.0)
    for k in range(N - 1, -1, -1):
        V = disc * (p * V[1:k + 2] + (1.0 - p) * V[:k + 1])
        if k % every == 0 and k > 0:
            V = np.maximum(V, K - S0 * u ** (2.0 * np.arange(k + 1) - k))
    return float(V[0])


# ---- the entry points as numpy calls -------------------------------------------------------------------------------------------

def fit_path(ctx, src, m, c, every, degree, D):
    """hh_lsm_fit_path_states -> (result, policy[date][2m + B])"""
    n_dates = c.n_steps // every
    policy = np.full(policy_shape(n_dates, degree), np.nan)
    assert policy.size == ctx.lib.hh_lsm_policy_elems(n_dates, M, degree)
    res, source = _ffi.hh_lsm_result(), src.source()
    ctx.check(ctx.lib.hh_lsm_fit_path_states(ctx.handle, C.byref(source), C.byref(m), C.byref(c), every, degree, D, C.byref(res),
                                             policy.ctypes.data))
    return res, policy


def value_path(ctx, src, m, c, every, policy, degree, D):
    """hh_lsm_policy_value_path -> result"""
    res, source = _ffi.hh_lsm_result(), src.source()
    policy = np.ascontiguousarray(policy)
    ctx.check(ctx.lib.hh_lsm_policy_value_path(ctx.handle, C.byref(source), C.byref(m), C.byref(c), every, policy.ctypes.data, degree,
                                               D, C.byref(res)))
    return res


def upper_bound(ctx, m, c, every, policy, degree, D, n_inner, inner_seed, want=True):
    """hh_lsm_upper_bound -> (result, cont[date][column], cont_se, pathwise_max)"""
    n_dates, n = c.n_steps // every, int(c.n_paths)
    cont, se, pmax = np.full((n_dates, n), np.nan), np.full((n_dates, n), np.nan), np.full(n, np.nan)
    res = _ffi.hh_bounds_result()
    policy = np.ascontiguousarray(policy)
    ctx.check(ctx.lib.hh_lsm_upper_bound(ctx.handle, C.byref(m), C.byref(c), every, policy.ctypes.data, degree, D, n_inner,
                                         inner_seed, C.byref(res), cont.ctypes.data if want else None, se.ctypes.data if want else None,
                                         pmax.ctypes.data if want else None))
    return res, cont, se, pmax
