"""Several correlated lognormal assets (include/hedgehog_mc.h, "Several correlated lognormal assets"): what the host and
the device tests share.

  * the cases of the issue — (a) three assets, (b) two, (e) eight with C_ij = 0.5^|i−j| — and their closed forms at 50
    digits: the call on a geometric index (lognormal), Margrabe's exchange option, Stulz's call on the minimum of two
    assets and the call on their maximum (the bivariate normal by quadrature), the discretely monitored geometric
    Asian on the geometric index; each also with every off-diagonal correlation set to 0;
  * the host's part restated in Python floats, operation for operation: the Cholesky factor (Cholesky–Banachiewicz,
    row by row) and the step's constants;
  * the draws of domain 6 from the oracle's host Philox, restated at 50 digits by hh_rng.h's formulas
    (tests/lognormal_exact_cases.box_muller);
  * a restatement of the step, the index and the five statistics, generic in the number type as
    tests/merton_cases.py's is: mpmath at 50 digits is the reference, Python floats are "the same formulas in fp64"
    whose distance from the 50-digit run is e64.  The bar of a statistic is euler_tangent_cases.path_bar(e64, A).
"""
import json
import math
import os

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex
from tests import path_payoff_cases as pc
from tests.lognormal_exact_cases import box_muller
from tests.path_bridge_cases import VA, _pick, _sqrt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assets_exact.json")
DOM_ASSETS = 6
DPS = ex.DPS
MAX = _ffi.HH_MAX_ASSETS
SUM, GEO, BEST, WORST = (_ffi.HH_INDEX_WEIGHTED_SUM, _ffi.HH_INDEX_GEOMETRIC, _ffi.HH_INDEX_BEST_OF,
                         _ffi.HH_INDEX_WORST_OF)
KINDS = (SUM, GEO, BEST, WORST)
GBM, EULER = _ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA


def decay_corr(d, rho=0.5):
    return [[rho ** abs(i - j) for j in range(d)] for i in range(d)]


CASE_A = dict(spots=[100.0, 90.0, 110.0], sigmas=[0.2, 0.35, 0.25], weights=[0.5, 0.3, 0.2],
              corr=[[1.0, 0.6, -0.3], [0.6, 1.0, 0.2], [-0.3, 0.2, 1.0]], r_drift=0.03, T=1.0)
CASE_B = dict(spots=[100.0, 95.0], sigmas=[0.3, 0.25], weights=[1.0, 1.0], corr=[[1.0, 0.7], [0.7, 1.0]], r_drift=0.03, T=1.0)
CASE_E = dict(spots=[100.0, 95.0, 105.0, 90.0, 110.0, 98.0, 102.0, 107.0],
              sigmas=[0.2, 0.25, 0.3, 0.22, 0.28, 0.18, 0.35, 0.24], weights=[0.125] * 8, corr=decay_corr(8),
              r_drift=0.03, T=1.0)
CASES = {"a": CASE_A, "b": CASE_B, "e": CASE_E}
ASIAN_SHAPE = (6, 2, 0)  # n_steps, monitor_every, include_start of the tabulated geometric Asian


def uncorrelated(case):
    d = len(case["spots"])
    return dict(case, corr=[[1.0 if i == j else 0.0 for j in range(d)] for i in range(d)])


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


# ---- closed forms at 50 digits ------------------------------------------------------------------------------------------

def _m(x):
    return mp.mpf(x)


def binormal(a, b, rho):
    """P(X <= a, Y <= b) of a standard bivariate normal with correlation rho, |rho| < 1: ∫_{−∞}^{a} φ(x)·Φ((b − ρx)/√(1 − ρ²)) dx"""
    a, b, rho = _m(a), _m(b), _m(rho)
    s = mp.sqrt(1 - rho * rho)
    lo = min(a, _m(-40))
    pts = [lo] + [t for t in (_m(-8), _m(-4), _m(-2), _m(0), _m(2), _m(4), _m(8)) if lo < t < a] + [a]
    return mp.quad(lambda x: mp.npdf(x) * mp.ncdf((b - rho * x) / s), pts)


def geometric_moments(case):
    """(mean, variance rate·T) of log Π S_i^{w_i} at T, and the drift and variance rate of the index's log"""
    S, sig, w = ([_m(t) for t in case[k]] for k in ("spots", "sigmas", "weights"))
    r, T, d = _m(case["r_drift"]), _m(case["T"]), len(case["spots"])
    x0 = mp.fsum(w[i] * mp.log(S[i]) for i in range(d))
    mu = mp.fsum(w[i] * (r - sig[i] * sig[i] / 2) for i in range(d))
    var = mp.fsum(w[i] * w[j] * sig[i] * sig[j] * _m(case["corr"][i][j]) for i in range(d) for j in range(d))
    return x0, mu, var, T


def _lognormal_call(mean, var, K, cp, D):
    sd = mp.sqrt(var)
    d2 = (mean - mp.log(_m(K))) / sd
    return D * cp * (mp.exp(mean + var / 2) * mp.ncdf(cp * (d2 + sd)) - _m(K) * mp.ncdf(cp * d2))


def geometric_index_vanilla(case, K, cp=1):
    with mp.workdps(DPS):
        x0, mu, var, T = geometric_moments(case)
        return +_lognormal_call(x0 + mu * T, var * T, K, cp, mp.exp(-_m(case["r_drift"]) * T))


def geometric_index_asian(case, K, cp, n_steps, every, include_start):
    """tests/path_payoff_cases.geometric_asian's law on the index: its log is a Brownian motion with drift"""
    with mp.workdps(DPS):
        x0, mu, var, T = geometric_moments(case)
        n = n_steps // every
        h = T * every / n_steps
        if include_start:
            mean = x0 + mu * h * n / 2
            v = var * h * n * (2 * n + 1) / (6 * _m(n + 1))
        else:
            mean = x0 + mu * h * (n + 1) / 2
            v = var * h * (n + 1) * (2 * n + 1) / (6 * _m(n))
        return +_lognormal_call(mean, v, K, cp, mp.exp(-_m(case["r_drift"]) * T))


def _two(case):
    assert len(case["spots"]) == 2
    S1, S2 = (_m(t) for t in case["spots"])
    s1, s2 = (_m(t) for t in case["sigmas"])
    return S1, S2, s1, s2, _m(case["corr"][0][1]), _m(case["r_drift"]), _m(case["T"])


def margrabe(case):
    """max(S_1 − S_2, 0) at T, discounted: S_1·Φ(d1) − S_2·Φ(d2), σ² = σ_1² + σ_2² − 2ρσ_1σ_2 (no dividends: r drops out)"""
    with mp.workdps(DPS):
        S1, S2, s1, s2, rho, r, T = _two(case)
        sd = mp.sqrt((s1 * s1 + s2 * s2 - 2 * rho * s1 * s2) * T)
        d1 = (mp.log(S1 / S2) + sd * sd / 2) / sd
        return +(S1 * mp.ncdf(d1) - S2 * mp.ncdf(d1 - sd))


def black_scholes(S, K, r, sig, T):
    sd = sig * mp.sqrt(T)
    d1 = (mp.log(S / K) + (r + sig * sig / 2) * T) / sd
    return S * mp.ncdf(d1) - K * mp.exp(-r * T) * mp.ncdf(d1 - sd)


def worst_of_call(case, K):
    """Stulz (1982): the call on the minimum of two assets"""
    with mp.workdps(DPS):
        S1, S2, s1, s2, rho, r, T = _two(case)
        K, sT = _m(K), mp.sqrt(T)
        sig = mp.sqrt(s1 * s1 + s2 * s2 - 2 * rho * s1 * s2)
        y1 = (mp.log(S1 / K) + (r + s1 * s1 / 2) * T) / (s1 * sT)
        y2 = (mp.log(S2 / K) + (r + s2 * s2 / 2) * T) / (s2 * sT)
        d = (mp.log(S1 / S2) + sig * sig * T / 2) / (sig * sT)
        r1, r2 = (s1 - rho * s2) / sig, (s2 - rho * s1) / sig
        return +(S1 * binormal(y1, -d, -r1) + S2 * binormal(y2, d - sig * sT, -r2)
                 - K * mp.exp(-r * T) * binormal(y1 - s1 * sT, y2 - s2 * sT, rho))


def best_of_call(case, K):
    """max = S_1 + S_2 − min, payoff by payoff: the two vanilla calls less the call on the minimum"""
    with mp.workdps(DPS):
        S1, S2, s1, s2, rho, r, T = _two(case)
        return +(black_scholes(S1, _m(K), r, s1, T) + black_scholes(S2, _m(K), r, s2, T) - worst_of_call(case, K))


def closed_forms(case_id, case):
    """name -> 50-digit price of every closed form the golden file holds for the case"""
    out = {}
    if case_id in ("a", "e"):
        out["geometric_call_K100"] = geometric_index_vanilla(case, 100.0, 1)
    if case_id == "a":
        out["geometric_asian_K100"] = geometric_index_asian(case, 100.0, 1, *ASIAN_SHAPE)
        out["geometric_put_K105"] = geometric_index_vanilla(case, 105.0, -1)
    if case_id == "b":
        out["margrabe"] = margrabe(case)
        out["worst_of_call_K100"] = worst_of_call(case, 100.0)
        out["best_of_call_K100"] = best_of_call(case, 100.0)
    return out


# the issue's table, computed there in double precision: (case, name) -> (closed form, ρ set to 0)
ISSUE_TABLE = {("a", "geometric_call_K100"): (7.27858, 5.65821), ("b", "margrabe"): (11.19288, 17.72208),
               ("b", "worst_of_call_K100"): (5.92711, 2.54467), ("b", "best_of_call_K100"): (15.92032, 19.30276),
               ("a", "geometric_asian_K100"): (4.90313, 3.80904)}


# ---- the host's part in Python floats --------------------------------------------------------------------------------------

def tri(i, j):
    return i * (i + 1) // 2 + j


def corr_defect(C):
    """csrc/hh_assets.h: corr_defect, on a nested list"""
    d = len(C)
    for i in range(d):
        for j in range(d):
            if not math.isfinite(C[i][j]) or not abs(C[i][j]) <= 1.0:
                return "range"
    for i in range(d):
        if C[i][i] != 1.0:
            return "diagonal"
    for i in range(d):
        for j in range(i):
            if C[i][j] != C[j][i]:
                return "asymmetric"
    return None


def cholesky_fp64(C):
    """csrc/hh_assets.h: cholesky — the same IEEE operations in the same order; None: not positive definite"""
    d = len(C)
    L = [0.0] * (d * (d + 1) // 2)
    for i in range(d):
        for j in range(i + 1):
            s = C[i][j]
            for k in range(j):
                s = s - L[tri(i, k)] * L[tri(j, k)]
            if j < i:
                L[tri(i, j)] = s / L[tri(j, j)]
            else:
                if not s > 0.0 or not math.isfinite(s):
                    return None
                L[tri(i, i)] = math.sqrt(s)
    return L


def constants_fp64(case, kind, n_steps, L):
    """csrc/hh_assets.h: asset_args -> (drift[d], A[packed], x0[d])"""
    d = len(case["spots"])
    dt = case["T"] / float(n_steps)
    sqrt_dt = math.sqrt(dt)
    drift, A, x0 = [], [0.0] * len(L), []
    for i in range(d):
        sig = case["sigmas"][i]
        drift.append((case["r_drift"] - 0.5 * sig * sig) * dt)
        for j in range(i + 1):
            A[tri(i, j)] = (sig * L[tri(i, j)]) * sqrt_dt
        lx = math.log(case["spots"][i])
        x0.append(lx + math.log(case["weights"][i]) if kind in (BEST, WORST) else lx)
    return drift, A, x0


# ---- the draws of domain 6 ----------------------------------------------------------------------------------------------------

def asset_normals(oracle, seeds, n_steps, d=MAX):
    """z[path][step][asset] at 50 digits: block (k, h, 0, 6) under the trajectory's seed gives (z_2h, z_2h+1)"""
    out = []
    with mp.workdps(DPS):
        for s in seeds:
            key = [int(s) & 0xFFFFFFFF, int(s) >> 32]
            rows = []
            for k in range(n_steps):
                z = []
                for h in range((d + 1) // 2):
                    z.extend(box_muller(oracle.philox([k, h, 0, DOM_ASSETS], key)))
                rows.append(z[:d])
            out.append(rows)
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def _expo(t):
    e = ex._exp(t.v)
    return VA(e, e * max(t.a, 1))


def _logv(t):
    l = ex._log(t.v)
    return VA(l, max(abs(l), t.a / abs(t.v)))


def _constants(case, kind, n_steps, num):
    """The Cholesky factor and the step's constants as values with magnitudes, in the header's order.  The factor enters
    the step with its own magnitude |L_ij|: what the fp64 factorisation loses against the exact one is in e64 (the two
    runs factor the matrix each in its own arithmetic), and a first-order magnitude carried through the recursion's
    squares and quotients overstates it by many orders at d = 8."""
    d = len(case["spots"])
    Lv = {}
    for i in range(d):
        for j in range(i + 1):
            s = num(case["corr"][i][j])
            for k in range(j):
                s = s - Lv[i, k] * Lv[j, k]
            Lv[i, j] = s / Lv[j, j] if j < i else ex._sqrt(s)
    L = {k: VA(v) for k, v in Lv.items()}
    dt = VA(num(case["T"]) / n_steps)
    sqrt_dt, half, r = _sqrt(dt), VA(num(0.5)), VA(num(case["r_drift"]))
    drift, A, x0 = [], {}, []
    for i in range(d):
        sig = VA(num(case["sigmas"][i]))
        drift.append((r - (half * sig) * sig) * dt)
        for j in range(i + 1):
            A[i, j] = (sig * L[i, j]) * sqrt_dt
        lx = ex._log(num(case["spots"][i]))
        x = VA(lx, max(abs(lx), 1))
        if kind in (BEST, WORST):
            lw = ex._log(num(case["weights"][i]))
            x = x + VA(lw, max(abs(lw), 1))
        x0.append(x)
    return drift, A, x0


def index_of(case, kind, x, num):
    """the pair (I, x) of the header's table, as VAs"""
    d = len(x)
    w = [VA(num(t)) for t in case["weights"]]
    if kind == SUM:
        I = w[0] * _expo(x[0])
        for i in range(1, d):
            I = I + w[i] * _expo(x[i])
        return I, _logv(I)
    if kind == GEO:
        xi = w[0] * x[0]
        for i in range(1, d):
            xi = xi + w[i] * x[i]
        return _expo(xi), xi
    xi = x[0]
    for i in range(1, d):
        xi = _pick(xi, x[i], kind == BEST)
    return _expo(xi), xi


def path_member(case, kind, num, z, mirror, monitor_every, include_start):
    """The five statistics of one member as VAs (rows of enum hh_path_stat): z[step][asset] the normals; the mirror takes
    −z.  A sum starts with its first term."""
    n_steps, d = len(z), len(case["spots"])
    drift, A, x = _constants(case, kind, n_steps, num)
    rows = None

    def take(S, xs):
        nonlocal rows
        rows = [S, xs, S, S, S] if rows is None else \
            [rows[0] + S, rows[1] + xs, _pick(rows[2], S, True), _pick(rows[3], S, False), S]

    if include_start:
        take(*index_of(case, kind, x, num))
    for k in range(n_steps):
        zk = [VA(num(-t if mirror else t)) for t in z[k]]
        for i in range(d):
            acc = drift[i]
            for j in range(i + 1):
                acc = acc + A[i, j] * zk[j]
            x[i] = x[i] + acc
        if (k + 1) % monitor_every == 0:
            take(*index_of(case, kind, x, num))
    return rows


def path_reference(case, kind, z, anti, monitor_every, include_start):
    """-> want [member][path][row] (mpf), e64 and A (float arrays [member][path][row])"""
    members, n = (2 if anti else 1), len(z)
    want = [[None] * n for _ in range(members)]
    e64, A = np.zeros((members, n, 5)), np.zeros((members, n, 5))
    with mp.workdps(DPS):
        for i in range(n):
            zf = [[float(t) for t in row] for row in z[i]]
            for m in range(members):
                ref = path_member(case, kind, mp.mpf, z[i], m == 1, monitor_every, include_start)
                f64 = path_member(case, kind, float, zf, m == 1, monitor_every, include_start)
                want[m][i] = [t.v for t in ref]
                A[m, i] = [float(t.a) for t in ref]
                e64[m, i] = [float(abs(mp.mpf(b.v) - a.v)) for a, b in zip(ref, f64)]
    return dict(want=want, e64=e64, A=A, members=members)


def index_numpy(case, kind):
    """the index at the spots in numpy doubles"""
    S, w = np.array(case["spots"]), np.array(case["weights"])
    if kind == SUM:
        return float(np.sum(w * S))
    if kind == GEO:
        return float(np.exp(np.sum(w * np.log(S))))
    return float(np.max(w * S)) if kind == BEST else float(np.min(w * S))


# ---- the C structs of a case, the cases of the device tests ------------------------------------------------------------------------

def assets_of(case, kind):
    return _ffi.make_assets(case["spots"], case["sigmas"], case["weights"], case["corr"], kind)


def model_of(case):
    """only T, r_drift and discount are read: the rest is set to values the single-asset entry points would reject"""
    return _ffi.make_model(S0=-1.0, V0=0.0, kappa=0.0, theta=0.0, sigma=float("nan"), rho=0.0, r=case["r_drift"], T=case["T"],
                           strike=0.0, cp=1.0, discount=case.get("discount"))


PATH_N = 257


def path_seeds():
    return np.arange(1, PATH_N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(13)


def path_case(d):
    """d assets of the path-by-path tests: positive weights (every row of every index kind is defined), correlations of
    both signs, T = 0.75"""
    spots = [100.0, 90.0, 110.0, 95.0, 105.0, 98.0, 102.0, 107.0][:d]
    sigmas = [0.2, 0.35, 0.25, 0.22, 0.28, 0.18, 0.3, 0.24][:d]
    weights = [1.0] if d == 1 else [0.5, 0.3, 0.2, 0.4, 0.1, 0.25, 0.15, 0.35][:d]
    corr = CASE_A["corr"] if d == 3 else decay_corr(d, -0.4 if d == 2 else 0.5)
    return dict(spots=spots, sigmas=sigmas, weights=weights, corr=corr, r_drift=0.03, T=0.75)


def payoff_list(case, kind):
    """one payoff of every kind 0 … 7, struck around the index at the spots"""
    I0 = index_numpy(case, kind)
    return [pc.payoff(pc.VANILLA, I0, 1.0), pc.payoff(pc.ARITH, 0.98 * I0, 1.0), pc.payoff(pc.GEOM, 1.01 * I0, -1.0),
            pc.payoff(pc.BARRIER, 0.95 * I0, 1.0, pc.DOWN_OUT, 0.9 * I0, 1.5), pc.payoff(pc.DCASH, 1.02 * I0, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 0.99 * I0, -1.0), pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0),
            pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FIXED, I0, 1.0)]
