"""Continuous extremes by Brownian bridge (include/hedgehog_mc.h, "CONTINUOUS MONITORING AND LOOKBACKS"): what the host
and the device tests share.

  * the payoff table of the two lookback kinds and of a barrier under either extremes mode, in numpy;
  * the closed forms under lognormal dynamics: Reiner–Rubinstein's up-and-out call, Goldman–Sosin–Gatto's floating
    lookback call;
  * the bridge uniforms from the oracle's host Philox;
  * a restatement of the Euler scheme (the formulas of oracle/euler_exact.py, values only) with the header's bridge
    formulas, generic in the number type: mpmath at 50 digits is the reference, Python floats are "the same formulas in
    fp64" whose distance from the 50-digit run sizes the bars, as in tests/euler_tangent_cases.py.

The bar of one member's CMAX_S or CMIN_S is  20·max(e64, ε·A).  A is a running magnitude: ε·A bounds, to first order,
the rounding error of any careful fp64 evaluation.  Along the trajectory it follows oracle/euler_exact.py's rules
(|x| + |y| for a sum, A_x·A_y for a product, max(|f|, |f'|·A_w) through a function).  Through the bridge formula:
  Δ = x1 − x0             A_Δ = A_x0 + A_x1
  Δ², g²                  2|Δ|·A_Δ, 2|g|·A_g — the first-order rule of a square, not A²: Δ is a small difference of two
                          numbers near log S0 and g the root of a variance near 0, where A_g is large because g is
                          small; A² would be hundreds of times the error any evaluation can make (a wider bar)
  L = −2 ln U             2·max(|ln U|, 1): U is exact, the logarithm's own error
  q = g²·dt               A_{g²}·dt
  R = Δ² + q·L            the sum of the two;  sqrt R: max(sqrt R, A_R / (2 sqrt R))
  M = ½(x0 + x1 ± sqrt R) half the sum of the three
  max / min               the larger of the operands' magnitudes (max is 1-Lipschitz in each operand)
  exp                     e·max(A, 1), as euler_exact.dexp forms it
"""
import math

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex
from tests import path_payoff_cases as pc

CMAX_S, CMIN_S = _ffi.HH_STAT_CMAX_S, _ffi.HH_STAT_CMIN_S
LB_FLOAT, LB_FIXED = _ffi.HH_PAYOFF_LOOKBACK_FLOAT, _ffi.HH_PAYOFF_LOOKBACK_FIXED
MONITORED, BRIDGE = _ffi.HH_EXTREMES_MONITORED, _ffi.HH_EXTREMES_BRIDGE
ROWS = {MONITORED: _ffi.HH_PATH_STATS, BRIDGE: _ffi.HH_PATH_STATS_BRIDGE}
DOM_BRIDGE = 3
EPS, FACTOR, MAX_UNUSABLE, MIN_CLIP_FRACTION = ex.EPS, 20.0, 0.02, 0.10


# ---- payoffs ---------------------------------------------------------------------------------------------------------

def extremes_of(stats, extremes):
    """(MAX, MIN) of every column as the payoffs of the mode read them"""
    return (stats[CMAX_S], stats[CMIN_S]) if extremes == BRIDGE else (stats[pc.MAX_S], stats[pc.MIN_S])


def payoff_from_stats(stats, q, n_mon, extremes):
    """The header's table for every kind under `extremes`: one IEEE operation per operation written there."""
    stats = np.asarray(stats, dtype=np.float64)
    mx, mn = extremes_of(stats, extremes)
    S_T = stats[pc.S_T]
    if q.kind == LB_FLOAT:
        return S_T - mn if q.cp > 0 else mx - S_T
    if q.kind == LB_FIXED:
        m = mx - q.strike if q.cp > 0 else q.strike - mn
        return np.where(m > 0.0, m, 0.0)
    five = stats[:_ffi.HH_PATH_STATS].copy()
    five[pc.MAX_S], five[pc.MIN_S] = mx, mn
    return pc.payoff_from_stats(five, q, n_mon)


# ---- closed forms under lognormal dynamics, continuous monitoring ------------------------------------------------------

def bs_call(S0, K, r, sigma, T):
    d1, d2 = pc.bs_d1_d2(S0, K, r, sigma, T)
    return S0 * pc.Phi(d1) - K * math.exp(-r * T) * pc.Phi(d2)


def up_and_out_call(S0, K, B, r, sigma, T):
    """Reiner–Rubinstein (1991), K < B, S0 < B, no rebate, no dividends: the density of S_T on paths that stay below B is
    the lognormal density minus its image reflected at B, weighted (B/S0)^(2λ−2), integrated over K < S_T < B."""
    sT, D = sigma * math.sqrt(T), math.exp(-r * T)
    lam = (r + 0.5 * sigma * sigma) / (sigma * sigma)
    x1 = math.log(S0 / K) / sT + lam * sT
    x2 = math.log(S0 / B) / sT + lam * sT
    y1 = math.log(B * B / (S0 * K)) / sT + lam * sT
    y2 = math.log(B / S0) / sT + lam * sT
    N, h = pc.Phi, B / S0
    return (S0 * (N(x1) - N(x2)) - K * D * (N(x1 - sT) - N(x2 - sT))
            - S0 * h ** (2 * lam) * (N(-y2) - N(-y1)) + K * D * h ** (2 * lam - 2) * (N(-y2 + sT) - N(-y1 + sT)))


def floating_lookback_call(S0, r, sigma, T):
    """Goldman–Sosin–Gatto (1979) at inception (running minimum = S0), r > 0, no dividends: E[e^{-rT}(S_T − min S)]."""
    sT, D = sigma * math.sqrt(T), math.exp(-r * T)
    a1 = (r + 0.5 * sigma * sigma) * T / sT
    a2 = a1 - sT
    k = sigma * sigma / (2 * r)
    return S0 * (pc.Phi(a1) - k * pc.Phi(-a1) - D * (1 - k) * pc.Phi(a2))


# ---- the bridge uniforms -----------------------------------------------------------------------------------------------

def u01(lo, hi):
    """hh_rng.h: u01_from_bits — ((w >> 12) + ½)·2⁻⁵², exact in fp64"""
    w = (int(hi) << 32) | int(lo)
    return ((w >> 12) + 0.5) * 2.0 ** -52


def bridge_uniforms(oracle, seeds, n_steps):
    """U[path][step] = (U1, U2): Philox block (k, 0, 0, 3) under the trajectory's seed"""
    out = np.empty((len(seeds), n_steps, 2))
    for i, s in enumerate(seeds):
        key = [int(s) & 0xFFFFFFFF, int(s) >> 32]
        for k in range(n_steps):
            c = oracle.philox([k, 0, 0, DOM_BRIDGE], key)
            out[i, k] = u01(c[0], c[1]), u01(c[2], c[3])
    return out


def increments_of(tiled, n, n_steps, ncomp):
    """tile-major REPLAY buffer of one tile, [step][comp][256] -> dW[path][step][comp]"""
    return np.ascontiguousarray(np.asarray(tiled).reshape(n_steps, ncomp, 256).transpose(2, 0, 1)[:n])


# ---- the restatement ---------------------------------------------------------------------------------------------------

class VA:
    """a value and its running magnitude"""
    __slots__ = ("v", "a")

    def __init__(self, v, a=None):
        self.v, self.a = v, abs(v) if a is None else a

    def __neg__(self):
        return VA(-self.v, self.a)

    def __add__(self, o):
        return VA(self.v + o.v, self.a + o.a)

    def __sub__(self, o):
        return VA(self.v - o.v, self.a + o.a)

    def __mul__(self, o):
        return VA(self.v * o.v, self.a * o.a)


def _sqrt(w):
    if not w.v > 0:
        return VA(w.v - w.v, ex._sqrt(w.a))
    s = ex._sqrt(w.v)
    return VA(s, max(s, w.a / (2 * s)))


def _square(x):
    return VA(x.v * x.v, 2 * abs(x.v) * x.a)


def _pick(a, b, larger):
    first = (a.v >= b.v) if larger else (a.v <= b.v)
    return VA(a.v if first else b.v, max(a.a, b.a))


def _bridge(x0, x1, q, L, sign):
    d = x1 - x0
    R = _square(d) + q * L
    root = _sqrt(R)
    m = x0 + x1 + (root if sign > 0 else -root)
    return VA(m.v / 2, m.a / 2)


def _neg2log(u, num):
    l = ex._log(num(u))
    return VA(-2 * l, 2 * max(abs(l), 1))


def walk(case, num, dW, U, mirror, record, swap=True):
    """One member of one path: dW[step][comp] and U[step] = (U1, U2) exact; mirror: −dW and, `swap`, L1 <-> L2.
    -> (S_T, CMAX_S, CMIN_S) as VA; the comparisons v > 0, K_v > 0 go on `record` as euler_exact's do."""
    heston = case["dynamics"] == "heston"
    c = {k: VA(num(case[k])) for k in ("S0", "V0", "kappa", "theta", "sigma", "r_drift")}
    dt, half = VA(num(case["T"]) / case["n_steps"]), VA(num(0.5))
    zero = VA(num(0.0))
    lx = ex._log(c["S0"].v)
    x = VA(lx, max(abs(lx), 1))  # euler_exact.dlog of an input
    v = c["V0"]
    drift = c["r_drift"] - (c["sigma"] * c["sigma"]) * half
    cmax = cmin = x
    for row, (u1, u2) in zip(dW, U):
        d = [VA(num(float(-t if mirror else t))) for t in row]
        x0 = x
        if heston:
            pos = v.v > 0
            record.append(("v", v.v, v.a, pos))
            vp = v if pos else zero
            Kx = x + (c["r_drift"] - vp * half) * dt
            Kv = v + (c["kappa"] * (c["theta"] - vp)) * dt
            if case["em_split"]:
                wpos = Kv.v > 0
                record.append(("Kv", Kv.v, Kv.a, wpos))
                w = Kv if wpos else zero
            else:
                w = vp
            g = _sqrt(w) if w.v > 0 else zero
            x = Kx + g * d[0]
            v = Kv + (c["sigma"] * g) * d[1]
        else:
            g = c["sigma"]
            x = (x + drift * dt) + g * d[0]
        q = _square(g) * dt
        L1, L2 = _neg2log(u1, num), _neg2log(u2, num)
        if mirror and swap:
            L1, L2 = L2, L1
        cmax = _pick(_pick(cmax, _bridge(x0, x, q, L1, +1), True), x, True)
        cmin = _pick(_pick(cmin, _bridge(x0, x, q, L2, -1), False), x, False)

    def expo(t):
        e = ex._exp(t.v)
        return VA(e, e * max(t.a, 1))
    return expo(x), expo(cmax), expo(cmin)


def reference(case, U):
    """Both runs on every path of case["dW"] with the uniforms U[path][step].  -> dict of arrays [member][path]:
    want (mpf: S_T, CMAX_S, CMIN_S), e64 and A (float, same three), wrong_cmax (mpf: the mirror's CMAX_S had it taken
    L1 — member 1 only), usable [path], clip_fraction."""
    members = 2 if case["antithetic"] else 1
    want = [[None] * len(U) for _ in range(members)]
    wrong = [None] * len(U)
    e64, A = np.zeros((members, len(U), 3)), np.zeros((members, len(U), 3))
    usable, clipped, total = np.zeros(len(U), dtype=bool), 0, 0
    with mp.workdps(ex.DPS):
        for i, (dW, u) in enumerate(zip(case["dW"], U)):
            rec_m, rec_6 = [], []
            for m in range(members):
                got_m = walk(case, mp.mpf, dW, u, m == 1, rec_m)
                got_6 = walk(case, float, dW, u, m == 1, rec_6)
                want[m][i] = [t.v for t in got_m]
                e64[m, i] = [float(abs(mp.mpf(b.v) - a.v)) for a, b in zip(got_m, got_6)]
                A[m, i] = [float(a.a) for a in got_m]
                if m == 1:
                    wrong[i] = walk(case, mp.mpf, dW, u, True, [], swap=False)[1].v
            usable[i] = ex._usable(rec_m, rec_6)
            vs = [t for t in rec_m if t[0] == "v"]
            clipped += sum(1 for t in vs if not t[3])
            total += len(vs)
    return dict(want=want, e64=e64, A=A, wrong_cmax=wrong, usable=usable, members=members,
                clip_fraction=clipped / total if total else 0.0)


def bar(e64, A):
    return FACTOR * np.maximum(e64, EPS * A)


# ---- the cases of the live-increment test ------------------------------------------------------------------------------

H252 = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r_drift=0.03, T=1.0)
CLIPPED = dict(H252, V0=0.01, kappa=0.5, theta=0.02, sigma=1.0, rho=-0.9)  # 2κθ < σ²
LIVE = {  # name -> (model, dynamics, em_split, n_steps, seed offset)
    "heston-split": (H252, "heston", 1, 16, 0),
    "heston-classic": (H252, "heston", 0, 16, 0),
    # (a mirror's maximum of this model lies at time 0 or in a clipped step, where no uniform enters, on about half of
    # all seeds; 43 is an offset with which 20 of the 32 mirrors' maxima depend on their uniform)
    "heston-classic-clipped": (CLIPPED, "heston", 0, 16, 43),
    "lognormal": (dict(H252, sigma=0.2), "lognormal", 1, 7, 0),
}
N_LIVE = 32


def live_seeds(name):
    """32 seeds per case; the offset is one for which the reference keeps every path (the host test asserts it on the
    oracle's increments)"""
    off = LIVE[name][4]
    return np.arange(1, N_LIVE + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(off)


def live_case(name, anti, dW):
    model, dyn, split, steps, _ = LIVE[name]
    return dict(model, dynamics=dyn, em_split=split, n_steps=steps, antithetic=anti, dW=dW)
