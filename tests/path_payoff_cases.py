"""Path-dependent payoffs (include/hedgehog_mc.h, "Path-dependent payoffs"): the numpy restatement of the payoff
table on the HH_PATH_STATS statistics, the closed forms that exist under lognormal dynamics, and the small builders
the host and the device tests share."""
import math

import numpy as np

from hedgehog_jl_amd import _ffi

SUM_S, SUM_X, MAX_S, MIN_S, S_T = (_ffi.HH_STAT_SUM_S, _ffi.HH_STAT_SUM_X, _ffi.HH_STAT_MAX_S, _ffi.HH_STAT_MIN_S,
                                   _ffi.HH_STAT_S_T)
VANILLA, ARITH, GEOM, BARRIER, DCASH, DASSET = (_ffi.HH_PAYOFF_VANILLA, _ffi.HH_PAYOFF_ASIAN_ARITH,
                                                _ffi.HH_PAYOFF_ASIAN_GEOM, _ffi.HH_PAYOFF_BARRIER,
                                                _ffi.HH_PAYOFF_DIGITAL_CASH, _ffi.HH_PAYOFF_DIGITAL_ASSET)
UP_OUT, UP_IN, DOWN_OUT, DOWN_IN = (_ffi.HH_BARRIER_UP_OUT, _ffi.HH_BARRIER_UP_IN, _ffi.HH_BARRIER_DOWN_OUT,
                                    _ffi.HH_BARRIER_DOWN_IN)


def payoff(kind, strike=100.0, cp=1.0, barrier_type=0, barrier=0.0, rebate=0.0, cash=0.0):
    q = _ffi.hh_path_payoff()
    q.kind, q.barrier_type, q.strike, q.cp, q.barrier, q.rebate, q.cash = kind, barrier_type, strike, cp, barrier, rebate, cash
    return q


def n_mon(n_steps, m, include_start):
    return n_steps // m + int(bool(include_start))


def monitored_rows(n_steps, m, include_start):
    """rows of a step-major grid [n_steps + 1][n] that are monitoring dates, in date order"""
    return ([0] if include_start else []) + list(range(m, n_steps + 1, m))


def payoff_from_stats(stats, q, n_mon):
    """The payoff q on every column of stats (HH_PATH_STATS, n): the header's table, one IEEE operation per operation
    written there (numpy's exp for the geometric average)."""
    stats = np.asarray(stats, dtype=np.float64)
    mT = q.cp * (stats[S_T] - q.strike)
    van = np.where(mT > 0.0, mT, 0.0)
    if q.kind == VANILLA:
        return van
    if q.kind == ARITH:
        m = q.cp * (stats[SUM_S] / float(n_mon) - q.strike)
        return np.where(m > 0.0, m, 0.0)
    if q.kind == GEOM:
        m = q.cp * (np.exp(stats[SUM_X] / float(n_mon)) - q.strike)
        return np.where(m > 0.0, m, 0.0)
    if q.kind == BARRIER:
        up = q.barrier_type in (UP_OUT, UP_IN)
        hit = stats[MAX_S] >= q.barrier if up else stats[MIN_S] <= q.barrier
        rebate = np.full_like(van, q.rebate)
        return np.where(hit, rebate, van) if q.barrier_type in (UP_OUT, DOWN_OUT) else np.where(hit, van, rebate)
    if q.kind == DCASH:
        return np.where(mT > 0.0, q.cash, 0.0)
    if q.kind == DASSET:
        return np.where(mT > 0.0, stats[S_T], 0.0)
    raise ValueError(q.kind)


def stats_of_grid(spot, logs, n_steps, m, include_start):
    """The five statistics from the step-major spot and log grids of hh_euler_grid, as the header defines them: the
    sums start with their first term and take one rounded addition per later date, in date order."""
    rows = monitored_rows(n_steps, m, include_start)
    sum_s, sum_x = spot[rows[0]].copy(), logs[rows[0]].copy()
    for r in rows[1:]:
        sum_s = sum_s + spot[r]
        sum_x = sum_x + logs[r]
    return np.stack([sum_s, sum_x, spot[rows].max(axis=0), spot[rows].min(axis=0), spot[n_steps]])


# ---- closed forms under lognormal dynamics -------------------------------------------------------------------------

def Phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def geometric_asian(S0, K, r, sigma, T, n_steps, m, include_start, cp):
    """Discretely monitored geometric Asian: log G is normal (a linear form of the Brownian path at the dates
    h, 2h, …, nh with h = m·T/n_steps, n = n_steps/m; with the start, date 0 too)."""
    h, n = m * T / n_steps, n_steps // m
    mu = r - 0.5 * sigma * sigma
    if include_start:
        mean = math.log(S0) + mu * h * n / 2.0
        var = sigma * sigma * h * n * (2 * n + 1) / (6.0 * (n + 1))
    else:
        mean = math.log(S0) + mu * h * (n + 1) / 2.0
        var = sigma * sigma * h * (n + 1) * (2 * n + 1) / (6.0 * n)
    sd = math.sqrt(var)
    d2 = (mean - math.log(K)) / sd
    d1 = d2 + sd
    return math.exp(-r * T) * cp * (math.exp(mean + var / 2.0) * Phi(cp * d1) - K * Phi(cp * d2))


def bs_d1_d2(S0, K, r, sigma, T):
    d1 = (math.log(S0 / K) + (r + 0.5 * sigma * sigma) * T) / (sigma * math.sqrt(T))
    return d1, d1 - sigma * math.sqrt(T)


def digital_cash(S0, K, r, sigma, T, cash, cp):
    return math.exp(-r * T) * cash * Phi(cp * bs_d1_d2(S0, K, r, sigma, T)[1])


def digital_asset(S0, K, r, sigma, T, cp):
    return S0 * Phi(cp * bs_d1_d2(S0, K, r, sigma, T)[0])
