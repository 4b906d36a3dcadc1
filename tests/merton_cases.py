"""Merton jump diffusion (include/hedgehog_mc.h, "Merton (1976) jump diffusion"): what the host and the device tests
share.

  * the closed forms at 50 digits: Merton's series of Black prices, the matching sum of Black digitals, and the exactly
    integrated truncated Carr–Madan integral (oracle/carr_madan_exact.py's quadrature on the Merton characteristic
    function), with the fp64 numpy restatement of the device's rule (oracle/carr_madan_fp64.py's nodes);
  * the Poisson inversion restated in exact arithmetic (mpmath) and, operation for operation, in Python floats;
  * the draws of domain 4 from the oracle's host Philox: the jump uniforms, and the jump normals restated at 50 digits
    by hh_rng.h's formulas (tests/lognormal_exact_cases.box_muller);
  * a restatement of the terminal law and of the path form, generic in the number type as tests/path_bridge_cases.py's
    walk is: mpmath at 50 digits is the reference, Python floats are "the same formulas in fp64" whose distance from the
    50-digit run is e64.

The bar of a state or statistic is euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A), imported.  A follows
oracle/euler_exact.py's rules (|x| + |y| for a sum, A_x·A_y for a product, max(|f|, |f'|·A_w) through a function)
through the one added sum and product of a jump: J = (σ_J·√N)·z + N·μ_J, x ← x + J.  A normal enters with its own
magnitude |z|.  The jump COUNT is no rounding matter: the fixtures keep every uniform at least MARGIN from every exact
cumulative boundary, so the 1e-16 of the fp64 sums cannot move it.
"""
import json
import math
import os

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import carr_madan_exact as cx
from oracle import euler_exact as ex
from tests import path_payoff_cases as pc
from tests.lognormal_exact_cases import box_muller
from tests.path_bridge_cases import VA, _pick, _sqrt, u01

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merton_exact.json")
DOM_JUMP = 4
MAX_COUNT, MAX_MEAN = _ffi.HH_JUMP_MAX_COUNT, _ffi.HH_JUMP_MAX_MEAN
MARGIN = 1e-9
DPS = ex.DPS
GBM, EXACT, EULER = _ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW, _ffi.HH_EULER_MARUYAMA
# the model of the issue's worked example: its series is 8.97843684569237157… at K = 105
BASE = dict(S0=100.0, sigma=0.2, r_drift=0.03, T=1.0, lam=0.8, mu_j=-0.1, sigma_j=0.15)


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


# ---- closed forms at 50 digits ----------------------------------------------------------------------------------------

def _ncdf(x):
    return mp.ncdf(x)


def kappa_bar(c):
    return mp.exp(mp.mpf(c["mu_j"]) + mp.mpf(c["sigma_j"]) ** 2 / 2) - 1


def series(c, K, cp, n_terms=400, digital_cash=None):
    """Σ_n e^{−λT}(λT)ⁿ/n! · (discounted Black price — or cash digital — on a lognormal with log-mean
    log S0 + (r − σ²/2 − λκ̄)T + n·μ_J and log-variance σ²T + n·σ_J²); the discount is e^{−rT} unless c has one."""
    with mp.workdps(DPS):
        S0, sig, r, T, lam, mu, sj = (mp.mpf(c[k]) for k in ("S0", "sigma", "r_drift", "T", "lam", "mu_j", "sigma_j"))
        D = mp.mpf(c["discount"]) if "discount" in c else mp.exp(-r * T)
        K, cp = mp.mpf(K), mp.mpf(cp)
        M0 = mp.log(S0) + (r - sig * sig / 2 - lam * kappa_bar(c)) * T
        w, total = mp.exp(-lam * T), mp.mpf(0)
        for n in range(n_terms):
            if n:
                w = w * lam * T / n
            M, V = M0 + n * mu, sig * sig * T + n * sj * sj
            if V == 0:
                itm = cp * (mp.exp(M) - K) > 0
                term = (mp.mpf(digital_cash) if itm else 0) if digital_cash is not None else max(cp * (mp.exp(M) - K), 0)
            else:
                sd = mp.sqrt(V)
                d2 = (M - mp.log(K)) / sd
                term = mp.mpf(digital_cash) * _ncdf(cp * d2) if digital_cash is not None else \
                    cp * (mp.exp(M + V / 2) * _ncdf(cp * (d2 + sd)) - K * _ncdf(cp * d2))
            total += w * term
        return +(D * total)


def black_scholes(c, K, cp):
    with mp.workdps(DPS):
        S0, sig, r, T = (mp.mpf(c[k]) for k in ("S0", "sigma", "r_drift", "T"))
        sd = sig * mp.sqrt(T)
        d1 = (mp.log(S0 / mp.mpf(K)) + (r + sig * sig / 2) * T) / sd
        return +(cp * (S0 * _ncdf(cp * d1) - mp.mpf(K) * mp.exp(-r * T) * _ncdf(cp * (d1 - sd))))


def log_cf(case):
    """tests/carr_madan_law_cases.py's law, exactly: log ϕ = (the normal law's log ϕ at the compensated drift) +
    λT·(exp(iμ_J·t − σ_J²t²/2) − 1) at t = v − i(α+1)"""
    lam, mu, sj = (cx._mpf(case[k]) for k in ("lam", "mu_j", "sigma_j"))
    p = {k: cx._mpf(case[k]) for k in ("S0", "K", "T", "r_drift", "discount", "alpha", "bound", "sigma")}
    p["compat_sqrt_alpha"] = False
    p["r_drift"] = p["r_drift"] - lam * kappa_bar(case)
    alpha = p["alpha"]

    def f(v):
        t = mp.mpc(v, -(alpha + 1))
        return cx.normal_log_cf(p, t) + lam * p["T"] * (mp.exp(mp.mpc(0, 1) * t * mu - sj * sj * t * t / 2) - 1)
    return f


def phi(case, u):
    """… and as hh_fourier.hip's MertonLaw forms it, in numpy complex128"""
    iu, T = 1j * u, case["T"]
    lam_kbar = case["lam"] * math.expm1(case["mu_j"] + 0.5 * case["sigma_j"] ** 2)
    mu = math.log(case["S0"]) + ((case["r_drift"] - 0.5 * case["sigma"] ** 2) - lam_kbar) * T
    sd = case["sigma"] * math.sqrt(T)
    jump = np.exp(case["mu_j"] * iu - (0.5 * case["sigma_j"] ** 2) * (u * u)) - 1.0
    return np.exp(mu * iu - (0.5 * sd * sd) * (u * u) + (case["lam"] * T) * jump)


def cm_bar(S0, e64):
    """tests/carr_madan_cases.price_bar's form"""
    from tests.carr_madan_cases import PRICE_FLOOR
    return max(PRICE_FLOOR * S0, 20.0 * e64)


# ---- the Poisson inversion ----------------------------------------------------------------------------------------------

def poisson_exact(U, m):
    """-> (N, the distance of U from the nearest exact cumulative boundary): the smallest n with U <= c_n in exact
    arithmetic (50 digits; U and m are doubles, taken exactly), HH_JUMP_MAX_COUNT at the latest.  The boundaries
    increase, so the nearest one is c_{N-1} or c_N."""
    with mp.workdps(DPS):
        U, m = mp.mpf(U), mp.mpf(m)
        p = mp.exp(-m)
        c, below = p, None
        for k in range(1, MAX_COUNT + 1):
            if U <= c:
                return k - 1, float(min(c - U, U - below if below is not None else c - U))
            below = c
            p = p * m / k
            c = c + p
        return MAX_COUNT, float(abs(U - c))


def poisson_fp64(U, m):
    """csrc/hh_jump.h's loop in Python floats: the same IEEE operations in the same order"""
    p = c = math.exp(-m)
    for k in range(1, MAX_COUNT + 1):
        if U <= c:
            return k - 1
        p = p * m / float(k)
        c = c + p
    return MAX_COUNT


def uniform_of(k):
    """((k) + ½)·2⁻⁵²: the uniform the device forms from a 52-bit k"""
    return (int(k) + 0.5) * 2.0 ** -52


# ---- the draws of domain 4 ----------------------------------------------------------------------------------------------

def _key(seed):
    return [int(seed) & 0xFFFFFFFF, int(seed) >> 32]


def terminal_uniforms(oracle, seed, path_offset, n):
    """U of trajectory g = path_offset + i of the stream keyed by `seed`: words 0, 1 of block (lo32 g, hi32 g, 1, 4)"""
    U = np.empty(n)
    for i in range(n):
        g = path_offset + i
        w = oracle.philox([g & 0xFFFFFFFF, g >> 32, 1, DOM_JUMP], _key(seed))
        U[i] = u01(w[0], w[1])
    return U


def terminal_normals(oracle, seed, path_offset, n):
    """(z1, z2) of the same trajectories at 50 digits, from block (lo32 g, hi32 g, 0, 4)"""
    with mp.workdps(DPS):
        return [box_muller(oracle.philox([(path_offset + i) & 0xFFFFFFFF, (path_offset + i) >> 32, 0, DOM_JUMP], _key(seed)))
                for i in range(n)]


def path_uniforms(oracle, seeds, n_steps):
    """U[i][k] of step k of the trajectory keyed by seeds[i]: block (k >> 1, 0, 0, 4), words 0, 1 for an even step,
    2, 3 for an odd one"""
    U = np.empty((len(seeds), n_steps))
    for i, s in enumerate(seeds):
        for k in range(n_steps):
            w = oracle.philox([k >> 1, 0, 0, DOM_JUMP], _key(s))
            U[i, k] = u01(w[2], w[3]) if k & 1 else u01(w[0], w[1])
    return U


def path_normals(oracle, seeds, N):
    """z[i][k]: the 50-digit jump normal of step k — the first of the pair of block (k, 1, 0, 4) — where N[i][k] > 0
    (the only steps whose block is drawn), None elsewhere"""
    with mp.workdps(DPS):
        return [[box_muller(oracle.philox([k, 1, 0, DOM_JUMP], _key(s)))[0] if N[i][k] > 0 else None
                 for k in range(len(N[i]))] for i, s in enumerate(seeds)]


def counts_of(U, mean, unusable=None):
    """the exact jump count of every uniform; every uniform keeps MARGIN from every cumulative boundary (asserted) — or,
    given a set `unusable`, the first index (the trajectory) of a uniform that does not is added to it"""
    N = np.empty(U.shape, dtype=np.int64)
    for idx, u in np.ndenumerate(U):
        N[idx], dist = poisson_exact(float(u), mean)
        if unusable is not None:
            if dist < MARGIN or N[idx] != poisson_fp64(float(u), mean):
                unusable.add(idx[0])
            continue
        assert dist >= MARGIN, (idx, float(u), mean, dist)
        assert N[idx] == poisson_fp64(float(u), mean)
    return N


# ---- the restatement ----------------------------------------------------------------------------------------------------

def _expo(t):
    e = ex._exp(t.v)
    return VA(e, e * max(t.a, 1))


def _model(case, num):
    """the scalars of a case as values with magnitudes, x0 = log S0 and the compensated drift (r − σ²/2) − λκ̄"""
    c = {k: VA(num(case[k])) for k in ("S0", "sigma", "r_drift", "T", "lam", "mu_j", "sigma_j")}
    half, one = VA(num(0.5)), VA(num(1.0))
    lx = ex._log(c["S0"].v)
    c["x0"] = VA(lx, max(abs(lx), 1))
    kbar = _expo(c["mu_j"] + (c["sigma_j"] * c["sigma_j"]) * half) - one
    c["drift"] = (c["r_drift"] - (c["sigma"] * c["sigma"]) * half) - c["lam"] * kbar
    return c


def _jump(c, N, z, num, mut=None):
    """J = (σ_J·√N)·z + N·μ_J; mut "sqrt_N" (qe_cases.SWEEP_MUTATIONS): N in place of √N"""
    n = VA(num(float(N)))
    return (c["sigma_j"] * (n if mut == "sqrt_N" else _sqrt(n))) * z + n * c["mu_j"]


def terminal_member(case, num, z1, z2, N, mirror):
    """S_T of one member of the terminal law as a VA: x_T = (σ√T)·z1 + m_T (+ J when N > 0); the mirror takes −z1, −z2"""
    c = _model(case, num)
    a, b = VA(num(z1)), VA(num(z2))
    if mirror:
        a, b = -a, -b
    x = (c["x0"] + c["drift"] * c["T"]) + (c["sigma"] * _sqrt(c["T"])) * a
    if N > 0:
        x = x + _jump(c, N, b, num)
    return _expo(x)


def terminal_reference(case, z, N):
    """-> want [member][path] (mpf S_T), e64 and A (float arrays [member][path])"""
    members = 2 if case["antithetic"] else 1
    n = len(z)
    want = [[None] * n for _ in range(members)]
    e64, A = np.zeros((members, n)), np.zeros((members, n))
    with mp.workdps(DPS):
        for i, ((z1, z2), Ni) in enumerate(zip(z, N)):
            for m in range(members):
                ref = terminal_member(case, mp.mpf, z1, z2, int(Ni), m == 1)
                f64 = terminal_member(case, float, float(z1), float(z2), int(Ni), m == 1)
                want[m][i], A[m, i] = ref.v, float(ref.a)
                e64[m, i] = float(abs(mp.mpf(f64.v) - ref.v))
    return dict(want=want, e64=e64, A=A, members=members)


def path_member(case, num, dW, N, z, mirror, monitor_every, include_start):
    """The five statistics of one member of the path form as VAs (rows of enum hh_path_stat): dW[step] exact (the
    device's own increments), N[step] the jump counts, z[step] the jump normals; the mirror takes −dW, the same N, −z.
    The step is oracle/euler_exact.gbm_path's, the statistics are the header's: a sum starts with its first term."""
    c = _model(case, num)
    dt = VA(num(case["T"]) / case["n_steps"])
    x = c["x0"]
    rows = None

    def take(S, xs):
        nonlocal rows
        rows = [S, xs, S, S, S] if rows is None else \
            [rows[0] + S, rows[1] + xs, _pick(rows[2], S, True), _pick(rows[3], S, False), S]

    if include_start:
        take(VA(num(case["S0"])), x)
    for k, d in enumerate(dW):
        d = VA(num(float(-d if mirror else d)))
        x = (x + c["drift"] * dt) + c["sigma"] * d
        if N[k] > 0:
            zk = VA(num(z[k]))
            x = x + _jump(c, int(N[k]), -zk if mirror else zk, num)
        if (k + 1) % monitor_every == 0:
            take(_expo(x), x)
    return rows


def path_reference(case, dW, N, z, monitor_every, include_start):
    """-> want [member][path][row] (mpf), e64 and A (float arrays [member][path][row])"""
    members = 2 if case["antithetic"] else 1
    n = len(dW)
    want = [[None] * n for _ in range(members)]
    e64, A = np.zeros((members, n, 5)), np.zeros((members, n, 5))
    with mp.workdps(DPS):
        for i in range(n):
            for m in range(members):
                ref = path_member(case, mp.mpf, dW[i], N[i], z[i], m == 1, monitor_every, include_start)
                f64 = path_member(case, float, dW[i], N[i], [None if t is None else float(t) for t in z[i]], m == 1,
                                  monitor_every, include_start)
                want[m][i] = [t.v for t in ref]
                A[m, i] = [float(t.a) for t in ref]
                e64[m, i] = [float(abs(mp.mpf(b.v) - a.v)) for a, b in zip(ref, f64)]
    return dict(want=want, e64=e64, A=A, members=members)


# ---- the C structs of a case ---------------------------------------------------------------------------------------------

def model_of(case, strike=100.0, cp=1.0):
    return _ffi.make_model(S0=case["S0"], V0=0.0, kappa=0.0, theta=0.0, sigma=case["sigma"], rho=0.0, r=case["r_drift"],
                           T=case["T"], strike=strike, cp=cp, discount=case.get("discount"))


def jump_of(case):
    return _ffi.make_jump(case["lam"], case["mu_j"], case["sigma_j"])


def payoff_list():
    """one payoff of every kind 0 … 7"""
    return [pc.payoff(pc.VANILLA, 100.0, 1.0), pc.payoff(pc.ARITH, 98.0, 1.0), pc.payoff(pc.GEOM, 101.0, -1.0),
            pc.payoff(pc.BARRIER, 95.0, 1.0, pc.DOWN_OUT, 80.0, 1.5), pc.payoff(pc.DCASH, 102.0, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 99.0, -1.0), pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0),
            pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FIXED, 100.0, 1.0)]


# ---- the cases of the device tests ---------------------------------------------------------------------------------------
# Their seeds are fixed here; tests/golden/make_merton_exact.py verifies on the CPU that every uniform they draw keeps
# MARGIN from every exact cumulative boundary and records the jump counts.

TERMINAL_SEED = 0x9E3779B97F4A7C15
TERMINAL_N = 513
TERMINAL_OFFSETS = (0, 1, 2**33 - 1)
TERMINAL_MEANS = (0.0, 0.5, 8.0)      # λ·T at T = 1
TERMINAL_SIZES = (1, 3, 255, 256, 257, 513)
PATH_N = 257
PATH_SHAPES = ((1, 1), (5, 1), (6, 1), (6, 3))  # (n_steps, monitor_every): 5 is the odd tail of the two-step loop
PATH_MEAN = 0.9                                  # λ·dt: N takes 0 … 4 within one case


def path_seeds():
    return np.arange(1, PATH_N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(11)


def terminal_case(mean, anti):
    return dict(BASE, lam=mean / BASE["T"], antithetic=anti)


def path_case(n_steps, anti):
    """λ such that λ·dt is PATH_MEAN up to rounding; jumps large enough to show in every row"""
    return dict(BASE, lam=PATH_MEAN * n_steps / BASE["T"], mu_j=-0.05, sigma_j=0.1, n_steps=n_steps, antithetic=anti)


def path_mean(case):
    """λ·dt as the library forms it: fl(λ · fl(T / n_steps))"""
    return case["lam"] * (case["T"] / case["n_steps"])
