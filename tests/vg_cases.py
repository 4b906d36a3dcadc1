"""Variance Gamma (include/hedgehog_mc.h, "Variance Gamma"): what the host and the device tests share.

  * the closed forms at 50 digits: the gamma-mixing integral of Black prices, Black–Scholes, and the exactly integrated
    truncated Carr–Madan integral (oracle/carr_madan_exact.py's graded sub-intervals on the Variance Gamma characteristic
    function) with the fp64 numpy restatement of the device's rule (oracle/carr_madan_fp64.py's nodes);
  * the host-formed constants and the Marsaglia–Tsang attempt loop of csrc/hh_vg.h restated generically in the number
    type, as tests/merton_cases.py's walk is: mpmath at 50 digits is the reference, Python floats in the header's
    operation order are "the same formulas in fp64", whose distance from the 50-digit run is e64;
  * the draws of domain 8 from the oracle's host Philox: the proposal normals restated at 50 digits by hh_rng.h's formulas
    (tests/lognormal_exact_cases.box_muller), U and U′ by path_bridge_cases.u01;
  * the terminal law and the path form on those variates.

The bar of a variate, a state or a statistic is euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A), imported; a
variate's bar is floored at 20·2⁻¹⁰⁷⁴, the spacing of fp64 where the boosted product underflows.  A follows
oracle/euler_exact.py's rules (|x| + |y| for a sum, A_x·A_y for a product, max(|f|, |f′|·A_w) through a function); a
normal enters with its own magnitude |z|, a uniform exactly.  Whether an attempt is ACCEPTED is no rounding matter: the
fixtures keep |rhs − log U| and |1 + c·z| at least MARGIN on every attempt (tests/golden/make_vg_exact.py asserts it), so
the 1e-15 of the fp64 sums cannot move a decision.
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
from tests.euler_tangent_cases import path_bar
from tests.lognormal_exact_cases import box_muller
from tests.path_bridge_cases import VA, _pick, _sqrt, u01

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vg_exact.json")
DOM_VG, DOM_EULER = 8, 0
MAX_ATTEMPTS = _ffi.HH_VG_MAX_ATTEMPTS
MARGIN = 1e-9
DPS = ex.DPS
TINY = 2.0 ** -1074
GBM, EXACT = _ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW
# the model of the issue's prices: calls 25.39428, 11.83230, 3.51079 at K = 80, 100, 120
BASE = dict(S0=100.0, sigma=0.2, r_drift=0.03, T=1.0, theta=-0.3, nu=0.5)
# (σ, θ, ν, T) of the analytic and Carr–Madan tests
PARAMS = ((0.2, -0.3, 0.5, 1.0), (0.2, -0.3, 0.5, 0.1), (0.12, -0.14, 0.2, 2.0))
STRIKES = (80.0, 100.0, 120.0)
HOST_SHAPES = (0.008, 0.25, 1.0, 4.7, 1e4)  # 1: the boost's boundary, not boosted
DEVICE_SHAPES = (0.008, 0.25, 4.7)
PATH_N = 513
PATH_SIZES = (257, 513)
PATH_STEPS = (1, 5, 8)
TERMINAL_SEED = 0x9E3779B97F4A7C15


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


def params_case(p):
    sigma, theta, nu, T = p
    return dict(BASE, sigma=sigma, theta=theta, nu=nu, T=T)


# ---- closed forms at 50 digits ----------------------------------------------------------------------------------------

def omega(c):
    sig, th, nu = (mp.mpf(c[k]) for k in ("sigma", "theta", "nu"))
    return mp.log(1 - th * nu - sig * sig * nu / 2) / nu


def discount_of(c):
    return c["discount"] if "discount" in c else math.exp(-c["r_drift"] * c["T"])


def mixing_price(c, K, cp):
    """E_G[discounted Black price on log-mean log S0 + (r + ω)T + θG and log-variance σ²G], G ~ Gamma(T/ν, ν), by
    mpmath's tanh-sinh rule at 50 digits of working precision on g = ν·e^u (the weight exp(a·u − e^u)/Γ(a) has no
    singularity).  The rule's own error is not 1e-50: against the exactly integrated Fourier integral at a bound whose
    tail is below 1e-16 it agrees to 8e-16 (tests/test_vg_host.py), five digits below the tightest bar it is used for."""
    with mp.workdps(DPS):
        S0, sig, r, T, th, nu = (mp.mpf(c[k]) for k in ("S0", "sigma", "r_drift", "T", "theta", "nu"))
        D, K, cp = mp.mpf(discount_of(c)), mp.mpf(K), mp.mpf(cp)
        a = T / nu
        m0 = mp.log(S0) + (r + omega(c)) * T

        def f(u):
            g = nu * mp.exp(u)
            w = mp.exp(a * u - mp.exp(u))
            M, V = m0 + th * g, sig * sig * g
            sd = mp.sqrt(V)
            d2 = (M - mp.log(K)) / sd
            if abs(d2) > 10000:  # Φ(±d2) is 0 or 1 to e^−5e7: the intrinsic value of the forward
                return w * max(cp * (mp.exp(M + V / 2) - K), 0)
            return w * cp * (mp.exp(M + V / 2) * mp.ncdf(cp * (d2 + sd)) - K * mp.ncdf(cp * d2))

        lo, top = -mp.mpf(150) / a - 10, mp.log(a + 160) + 2
        pts = [lo, mp.log(a) - 3, mp.log(a), mp.log(a) + 1, top]
        return +(D * mp.quad(f, pts, maxdegree=12) / mp.gamma(a))


def black_scholes(c, K, cp, vol=None):
    with mp.workdps(DPS):
        S0, r, T = (mp.mpf(c[k]) for k in ("S0", "r_drift", "T"))
        sig = mp.mpf(c["sigma"] if vol is None else vol)
        sd = sig * mp.sqrt(T)
        d1 = (mp.log(S0 / mp.mpf(K)) + (r + sig * sig / 2) * T) / sd
        return +(cp * (S0 * mp.ncdf(cp * d1) - mp.mpf(K) * mp.exp(-r * T) * mp.ncdf(cp * (d1 - sd))))


def log_cf(case):
    """tests/carr_madan_law_cases.py's law, exactly: log ϕ = it·(log S0 + (r + ω)T) − (T/ν)·log(1 − θν·it + σ²ν·t²/2) at
    t = v − i(α+1)"""
    p = {k: cx._mpf(case[k]) for k in ("S0", "K", "T", "r_drift", "alpha", "sigma", "theta", "nu")}
    alpha, a = p["alpha"], p["T"] / p["nu"]
    mu = mp.log(p["S0"]) + (p["r_drift"] + omega(case)) * p["T"]

    def f(v):
        t = mp.mpc(v, -(alpha + 1))
        it = mp.mpc(0, 1) * t
        base = 1 - p["theta"] * p["nu"] * it + p["sigma"] ** 2 * p["nu"] * t * t / 2
        return mu * it - a * mp.log(base)
    return f


def cm_tail_bound(case):
    """An upper bound of what the truncation leaves out, beyond ±bound: |ϕ| <= |ϕ(−i(α+1))|·(|base(v)|/base(0))^(−T/ν) with
    |base(v)| >= σ²ν·v²/2 − |Re base(0) − 1|, and |1/den| <= 1/v², integrated in closed form with the first term alone."""
    with mp.workdps(DPS):
        p = {k: cx._mpf(case[k]) for k in ("S0", "K", "T", "r_drift", "alpha", "sigma", "theta", "nu", "bound", "discount")}
        a, al, B = p["T"] / p["nu"], p["alpha"], p["bound"]
        mu = mp.log(p["S0"]) + (p["r_drift"] + omega(case)) * p["T"]
        q = p["sigma"] ** 2 * p["nu"] / 2
        # for v >= B: |base| >= q·v² − q(1+α)² − |θ|ν(1+α) − 1 >= (q/2)·v² once B is large enough (asserted)
        assert q * B * B / 2 >= q * (1 + al) ** 2 + abs(p["theta"]) * p["nu"] * (1 + al) + 1
        amp = mp.exp(mu * (1 + al))  # |exp(i t μ)| on the contour
        tail = amp * (q / 2) ** (-a) * B ** (-2 * a - 1) / (2 * a + 1)  # ∫_B^∞ (q v²/2)^(−a) v^(−2) dv
        return +(2 * tail * p["discount"] * mp.exp(-al * mp.log(p["K"])) / (2 * mp.pi))


def phi(case, u):
    """… and as hh_fourier.hip's VgLaw forms it, in numpy complex128"""
    iu, T = 1j * u, case["T"]
    th_nu, half_s2nu = case["theta"] * case["nu"], (0.5 * (case["sigma"] * case["sigma"])) * case["nu"]
    om = math.log((1.0 - th_nu) - half_s2nu) / case["nu"]
    mu = math.log(case["S0"]) + (case["r_drift"] + om) * T
    base = 1.0 - th_nu * iu + half_s2nu * (u * u)
    return np.exp(mu * iu - (T / case["nu"]) * np.log(base))


def cm_bar(case, e64):
    """tests/carr_madan_cases.price_bar's form, max(1e-14·S0, 20·e64), with the power's own term beside e64: the exponent
    (T/ν)·log(base) is rounded at (T/ν)·|log base|·2⁻⁵² relative per node, |log base| <= log(1 + |θ|ν·B + σ²ν·B²/2) with
    B = bound + α + 1, and the nodes' weights sum to at most the price's own size, S0."""
    from tests.carr_madan_cases import PRICE_FLOOR
    B = case["bound"] + case["alpha"] + 1.0
    logb = math.log(1.0 + abs(case["theta"]) * case["nu"] * B + 0.5 * case["sigma"] ** 2 * case["nu"] * B * B)
    power = (case["T"] / case["nu"]) * logb * 2.0 ** -52 * case["S0"]
    return max(PRICE_FLOOR * case["S0"], 20.0 * e64, power)


# ---- the sampler, restated ------------------------------------------------------------------------------------------------

def _logv(w):
    l = ex._log(w.v)
    return VA(l, max(abs(l), w.a / w.v))


def _expo(t):
    e = ex._exp(t.v)
    return VA(e, e * max(t.a, 1))


def vg_args(num, sigma, r_drift, theta, nu, span):
    """csrc/hh_vg.h's vg_args in the number type, one operation per operation written there; -> dict of VA and `boost`"""
    one, half = VA(num(1.0)), VA(num(0.5))
    sig, r, th, n_, sp = (VA(num(t)) for t in (sigma, r_drift, theta, nu, span))
    arg = (one - th * n_) - (half * (sig * sig)) * n_
    la = _logv(arg)
    om = VA(la.v / n_.v, la.a / n_.v)
    a = sp.v / n_.v
    boost = a < 1
    a1 = a + 1 if boost else a
    if num is float:
        d = a1 - 1.0 / 3.0
        c, inv_a = 1.0 / math.sqrt(9.0 * d), 1.0 / a
    else:
        d = a1 - mp.mpf(1.0 / 3.0)  # the double 1.0/3.0, taken exactly
        c, inv_a = 1 / mp.sqrt(9 * d), 1 / a
    return dict(d=VA(d), c=VA(c), inv_a=VA(inv_a), nu_d=VA(n_.v * d), theta=th, sigma=sig, drift=(r + om) * sp, boost=boost)


def gamma_walk(g, draws, num):
    """csrc/hh_vg.h's gamma_mt on `draws` = [(z, U, U′)] (z in the number type, the uniforms doubles) ->
    (variate VA, attempts made, the smallest decision margin met).  Runs out of draws: ValueError."""
    last, margin = VA(num(0.0)), float("inf")
    half, one = VA(num(0.5)), VA(num(1.0))
    for t in range(MAX_ATTEMPTS):
        if t >= len(draws):
            raise ValueError("the walk asks for more attempts than there are draws")
        z, U, Ub = draws[t]
        z = VA(num(z))
        x = one + g["c"] * z
        margin = min(margin, abs(float(x.v)))
        v = (x * x) * x
        if v.v > 0:
            rhs = (((half * z) * z + g["d"]) - g["d"] * v) + g["d"] * _logv(v)
            val = g["nu_d"] * v
            if g["boost"]:
                val = val * _expo(_logv(VA(num(U if Ub is None else Ub))) * g["inv_a"])
            last = val
            lu = ex._log(num(U))
            margin = min(margin, abs(float(rhs.v - lu)))
            if lu < rhs.v:
                return last, t + 1, margin
    return last, MAX_ATTEMPTS, margin


def variate_reference(g50, g64, draws50):
    """One variate at 50 digits and in fp64 on the same draws -> dict(want, bar, attempts, margin); the fp64 walk must make
    the same decisions"""
    with mp.workdps(DPS):
        ref, n, margin = gamma_walk(g50, draws50, mp.mpf)
        f64, n64, _ = gamma_walk(g64, [(float(draws50[t][0]),) + tuple(draws50[t][1:]) for t in range(n)], float)
        assert n == n64, (n, n64)
        e64 = float(abs(mp.mpf(f64.v) - ref.v))
        return dict(want=ref.v, A=float(ref.a), e64=e64, bar=max(float(path_bar(e64, float(ref.a))), 20.0 * TINY),
                    attempts=n, margin=margin, va=ref, va64=f64)


# ---- the draws of domain 8 --------------------------------------------------------------------------------------------------

def _key(seed):
    return [int(seed) & 0xFFFFFFFF, int(seed) >> 32]


class Attempts:
    """The draws of one variate, block by block as the walk asks for them: ctr_z(t) and ctr_u(t) the two counters of attempt t"""

    def __init__(self, oracle, seed, ctr_z, ctr_u):
        self.oracle, self.key, self.ctr_z, self.ctr_u, self.got = oracle, _key(seed), ctr_z, ctr_u, []

    def __len__(self):
        return MAX_ATTEMPTS

    def __getitem__(self, t):
        if t >= MAX_ATTEMPTS:
            raise IndexError(t)
        while len(self.got) <= t:
            k = len(self.got)
            z = box_muller(self.oracle.philox(self.ctr_z(k), self.key))[0]
            w = self.oracle.philox(self.ctr_u(k), self.key)
            self.got.append((z, u01(w[0], w[1]), u01(w[2], w[3])))
        return self.got[t]


def terminal_attempts(oracle, seed, g):
    lo, hi = g & 0xFFFFFFFF, g >> 32
    return Attempts(oracle, seed, lambda t: [lo, hi, 2 * t, DOM_VG], lambda t: [lo, hi, 2 * t + 1, DOM_VG])


def terminal_normal(oracle, seed, g):
    return box_muller(oracle.philox([g & 0xFFFFFFFF, g >> 32, 2 * MAX_ATTEMPTS, DOM_VG], _key(seed)))[0]


def step_attempts(oracle, seed, k):
    return Attempts(oracle, seed, lambda t: [k, t, 0, DOM_VG], lambda t: [k, t, 1, DOM_VG])


def step_normals(oracle, seed, n_steps):
    """z_B of steps 0 .. n_steps − 1: the pair of block (k >> 1, 0, 0, 0), first normal for an even k, second for an odd one"""
    out = []
    for h in range((n_steps + 1) // 2):
        out += list(box_muller(oracle.philox([h, 0, 0, DOM_EULER], _key(seed))))
    return out[:n_steps]


# ---- the terminal law and the path form on those variates ------------------------------------------------------------------

def increment(g, G, zB, mirror):
    z = -zB if mirror else zB
    return (g["drift"] + g["theta"] * G) + (g["sigma"] * _sqrt(G)) * z


def x0_of(case, num):
    lx = ex._log(num(case["S0"]))
    return VA(lx, max(abs(lx), 1))


def path_rows(case, num, g, G, zB, mirror, monitor_every, include_start):
    """the five statistics of one member (rows of enum hh_path_stat) as VAs: G[k] the step's variate, zB[k] its normal"""
    x = x0_of(case, num)
    rows = None

    def take(S, xs):
        nonlocal rows
        rows = [S, xs, S, S, S] if rows is None else \
            [rows[0] + S, rows[1] + xs, _pick(rows[2], S, True), _pick(rows[3], S, False), S]

    if include_start:
        take(VA(num(case["S0"])), x)
    for k in range(len(G)):
        x = x + increment(g, G[k], VA(num(zB[k])), mirror)
        if (k + 1) % monitor_every == 0:
            take(_expo(x), x)
    return rows


class PathDraws:
    """Everything of a (shape per draw, n_steps) pair that does not depend on the monitoring or the mirror: the constants,
    the variates at 50 digits and in fp64, the attempt counts, the normals.  terminal=True: the terminal law's draws."""

    def __init__(self, oracle, case, n_steps, n, seeds, terminal=False, path_offset=0):
        self.case, self.n_steps = case, n_steps
        with mp.workdps(DPS):
            span = case["T"] if terminal else case["T"] / n_steps  # fl(T / n_steps), as make_args forms dt
            self.g50 = vg_args(mp.mpf, case["sigma"], case["r_drift"], case["theta"], case["nu"], span)
            self.g64 = vg_args(float, case["sigma"], case["r_drift"], case["theta"], case["nu"], span)
            self.G50, self.G64, self.attempts, self.margin, self.zB = [], [], [], float("inf"), []
            for i in range(n):
                row50, row64, att = [], [], []
                for k in range(n_steps):
                    src = terminal_attempts(oracle, seeds[0], path_offset + i) if terminal else step_attempts(oracle, seeds[i], k)
                    r = variate_reference(self.g50, self.g64, src)
                    row50.append(r["va"]); row64.append(r["va64"]); att.append(r["attempts"])
                    self.margin = min(self.margin, r["margin"])
                self.G50.append(row50); self.G64.append(row64); self.attempts.append(att)
                self.zB.append([terminal_normal(oracle, seeds[0], path_offset + i)] if terminal
                               else step_normals(oracle, seeds[i], n_steps))

    def reference(self, anti, monitor_every, include_start):
        """-> want [member][path][row] (mpf), bars (float array [member][path][row])"""
        members = 2 if anti else 1
        n = len(self.G50)
        want = [[None] * n for _ in range(members)]
        e64, A = np.zeros((members, n, 5)), np.zeros((members, n, 5))
        with mp.workdps(DPS):
            for i in range(n):
                for m in range(members):
                    ref = path_rows(self.case, mp.mpf, self.g50, self.G50[i], self.zB[i], m == 1, monitor_every, include_start)
                    f64 = path_rows(self.case, float, self.g64, self.G64[i], [float(t) for t in self.zB[i]], m == 1,
                                    monitor_every, include_start)
                    want[m][i] = [t.v for t in ref]
                    A[m, i] = [float(t.a) for t in ref]
                    e64[m, i] = [float(abs(mp.mpf(b.v) - a.v)) for a, b in zip(ref, f64)]
        return dict(want=want, bars=path_bar(e64, A), members=members)


# ---- the C structs of a case ---------------------------------------------------------------------------------------------

def model_of(case, strike=100.0, cp=1.0):
    return _ffi.make_model(S0=case["S0"], V0=0.0, kappa=0.0, theta=0.0, sigma=case["sigma"], rho=0.0, r=case["r_drift"],
                           T=case["T"], strike=strike, cp=cp, discount=case.get("discount"))


def vg_of(case):
    return _ffi.make_vg(case["theta"], case["nu"])


def payoff_list():
    """one payoff of every kind 0 … 7"""
    return [pc.payoff(pc.VANILLA, 100.0, 1.0), pc.payoff(pc.ARITH, 98.0, 1.0), pc.payoff(pc.GEOM, 101.0, -1.0),
            pc.payoff(pc.BARRIER, 95.0, 1.0, pc.DOWN_OUT, 80.0, 1.5), pc.payoff(pc.DCASH, 102.0, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 99.0, -1.0), pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0),
            pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FIXED, 100.0, 1.0)]


def path_seeds():
    return np.arange(1, PATH_N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(8)


def shape_case(shape, n_steps):
    """ν such that (T/n_steps)/ν is `shape` up to rounding; θ < 0 keeps 1 − θν − σ²ν/2 = 1 + 0.28·ν positive at any ν"""
    return dict(BASE, nu=BASE["T"] / n_steps / shape)
