"""The Crank–Nicolson scheme of hh_fd_solve (include/hedgehog_mc.h) restated serially, generically in the number type,
the cases the host and device tests price, and the bars they hold results to.

`restate(FP64, …)` runs in Python floats (IEEE double, one rounding per operation), `restate(MP50, …)` at 50 digits.
Per run and output, e64 = |fp64 run − 50-digit run| and

    bar = path_bar(e64, A) = 20 · max(e64, ε·A),   ε = 2⁻⁵²            (tests/euler_tangent_cases.py: the project's form)

with A the size of the terms the output differences: K for the price, K/(S0·h) for the delta, K/(S0²·h²) for the gamma.
Nothing in a bar comes from the device.  The 50-digit results of the device test's runs are committed
(tests/golden/fd_exact.json, written by tests/golden/make_fd_exact.py); tests/test_fd_host.py regenerates a sample.

The restatement is a plain Thomas solve per step (Brennan–Schwartz for American exercise: a put eliminates the
super-diagonal from the top row down and substitutes upwards with the max, a call mirrors it).  The device scans the
same two recurrences; the host program tests/c/fd_host_check.cpp runs csrc/hh_fd.h's serial step."""
import json
import math
import os

import mpmath as mp
import numpy as np

from tests.euler_tangent_cases import EPS, path_bar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fd_exact.json")
DPS = 50
EUROPEAN, AMERICAN = 0, 1

# (S0, K, r, σ, T)
CASES = [(100.0, 100.0, 0.05, 0.2, 1.0), (100.0, 90.0, 0.03, 0.3, 0.5), (100.0, 115.0, 0.06, 0.15, 2.0),
         (50.0, 55.0, 0.01, 0.6, 0.25), (100.0, 100.0, 0.08, 0.1, 1.0), (100.0, 100.0, 0.0, 0.2, 1.0)]
SIDES = [(cp, style) for cp in (1.0, -1.0) for style in (EUROPEAN, AMERICAN)]


class FP64:
    num = float
    exp = staticmethod(math.exp)
    log = staticmethod(math.log)


class MP50:
    num = staticmethod(lambda x: mp.mpf(x))
    exp = staticmethod(lambda x: mp.exp(x))
    log = staticmethod(lambda x: mp.log(x))


def half_width(S0, K, r, sigma, T, n_std=6.0):
    """W as hedgehog_jl_amd.pde.fd_inputs forms it, in fp64"""
    return n_std * sigma * math.sqrt(T) + abs(math.log(K / S0)) + abs(r - 0.5 * sigma * sigma) * T


# The five mutations of the issue: each, applied here, must make the device test fail (recorded in DESIGN §5.11).
MUTATIONS = ("no_max", "american_put_end_discounted", "lo_up_swapped", "theta_one", "gamma_without_d1")


def restate(F, S0, K, cp, sigma, r, T, W, style, M, N, R, mutation=None):
    """(price, delta, gamma) of one option; the seven scalars are doubles, converted exactly"""
    c = F.num
    S0, K, cp, sigma, r, T, W = (c(v) for v in (S0, K, cp, sigma, r, T, W))
    american = style == AMERICAN
    half = M // 2
    h = W / half
    a = sigma * sigma / 2
    b = r - a
    lo = a / (h * h) - b / (2 * h)
    di = -2 * a / (h * h) - r
    up = a / (h * h) + b / (2 * h)
    if mutation == "lo_up_swapped":
        lo, up = up, lo
    x0 = F.log(S0)
    S = [F.exp(x0 + (j - half) * h) for j in range(M + 1)]
    zero = c(0)
    g = [max(cp * (s - K), zero) for s in S]
    V = list(g)
    dt = T / N
    tau = zero
    pivots = {}

    def step(k, theta):
        nonlocal tau, V
        tk = theta * k
        A, B, C, e = tk * lo, 1 - tk * di, tk * up, (1 - theta) * k
        y = [None] * (M + 1)
        for j in range(1, M):
            y[j] = V[j] + e * ((lo * V[j - 1] + di * V[j]) + up * V[j + 1])
        tau = tau + k
        disc = F.exp(-r * tau)
        W_ = [None] * (M + 1)
        put = cp < 0
        if put:
            W_[M] = zero
            W_[0] = K - S[0] if american and mutation != "american_put_end_discounted" else K * disc - S[0]
        else:
            W_[0] = zero
            W_[M] = S[M] - K * disc
        key = (k, theta)
        if key not in pivots:  # the factorisation depends on (k, θ) alone
            piv, mul = [None] * (M + 1), [None] * (M + 1)
            if put:
                piv[M - 1] = B
                for j in range(M - 2, 0, -1):
                    mul[j] = C / piv[j + 1]
                    piv[j] = B - mul[j] * A
            else:
                piv[1] = B
                for j in range(2, M):
                    mul[j] = A / piv[j - 1]
                    piv[j] = B - mul[j] * C
            pivots[key] = (piv, mul)
        piv, mul = pivots[key]
        use_max = american and mutation != "no_max"
        if put:
            y[M - 1] = y[M - 1] + C * W_[M]
            for j in range(M - 2, 0, -1):
                y[j] = y[j] + mul[j] * y[j + 1]
            for j in range(1, M):
                x = (y[j] + A * W_[j - 1]) / piv[j]
                W_[j] = max(x, g[j]) if use_max else x
        else:
            y[1] = y[1] + A * W_[0]
            for j in range(2, M):
                y[j] = y[j] + mul[j] * y[j - 1]
            for j in range(M - 1, 0, -1):
                x = (y[j] + C * W_[j + 1]) / piv[j]
                W_[j] = max(x, g[j]) if use_max else x
        V = W_

    half_c, one = c(1) / 2, c(1)
    for n in range(N):
        if n < R or mutation == "theta_one":
            if n < R:
                step(dt / 2, one)
                step(dt / 2, one)
            else:
                step(dt, one)
        else:
            step(dt, half_c)
    ctr = half
    d1 = (V[ctr + 1] - V[ctr - 1]) / (2 * h)
    d2 = (V[ctr + 1] - 2 * V[ctr] + V[ctr - 1]) / (h * h)
    gamma = d2 / (S0 * S0) if mutation == "gamma_without_d1" else (d2 - d1) / (S0 * S0)
    return V[ctr], d1 / S0, gamma


def magnitudes(S0, K, W, M):
    """A of the three outputs"""
    h = W / (M // 2)
    return np.array([K, K / (S0 * h), K / (S0 * S0 * h * h)])


# ---- the runs of the device test ---------------------------------------------------------------------------------------

# every (N, R) with N in {1, 2, 3, 50} and R in {0, 2, N} that has R <= N
NR_ALL = [(1, 0), (1, 1), (2, 0), (2, 2), (3, 0), (3, 2), (3, 3), (50, 0), (50, 2), (50, 50)]
NR_LARGE = [(3, 2), (50, 2)]
# both sides of every boundary of the kernel's layout (64·C nodes per wave, C = 1, 2, 4, 8, 16; four waves with
# C = 8, 16 above 1024), each form's largest M and that M + 2, and sizes that fill no lane evenly
M_SMALL = [4, 8, 62, 64, 66, 128, 130, 200, 256, 258]
M_LARGE = [512, 514, 1024, 1026, 2048, 2050, 4096]
NARROW = 0.5   # n_std of the runs whose lower end lies in the continuation region: the end's value matters there


def run_list():
    """[(case index, cp, style, M, N, R, n_std)] — the cases rotate over the sizes; M = 200 prices all of them"""
    runs = []
    for i, M in enumerate(M_SMALL + M_LARGE):
        for N, R in (NR_ALL if M in M_SMALL else NR_LARGE):
            for cp, style in SIDES:
                runs.append((i % len(CASES), cp, style, M, N, R, 6.0))
    for ci in range(len(CASES)):
        for cp, style in SIDES:
            if (ci, cp, style, 200, 50, 2, 6.0) not in runs:
                runs.append((ci, cp, style, 200, 50, 2, 6.0))
    for ci in (0, 1, 4):
        for M, N, R in ((64, 50, 2), (130, 50, 0)):
            for cp, style in SIDES:
                runs.append((ci, cp, style, M, N, R, NARROW))
    return runs


def scalars(run):
    """(S0, K, cp, σ, r, T, W, style, M, N, R) of a run: what hh_fd_solve and restate receive"""
    ci, cp, style, M, N, R, n_std = run
    S0, K, r, sigma, T = CASES[ci]
    return S0, K, cp, sigma, r, T, half_width(S0, K, r, sigma, T, n_std), style, M, N, R


def reference(run, mutation=None):
    """(50-digit results as mpf, e64 as floats)"""
    args = scalars(run)
    got64 = restate(FP64, *args, mutation=mutation)
    with mp.workdps(DPS):
        exact = restate(MP50, *args, mutation=mutation)
        e64 = [float(abs(mp.mpf(a) - b)) for a, b in zip(got64, exact)]
    return exact, e64


def load_golden():
    doc = json.load(open(GOLDEN))
    out = {}
    with mp.workdps(DPS):
        for rec in doc["runs"]:
            key = (rec["case"], rec["cp"], rec["style"], rec["M"], rec["N"], rec["R"], rec["n_std"])
            out[key] = ([mp.mpf(s) for s in rec["ref"]], [float.fromhex(x) for x in rec["e64"]])
    return out


def bars(run, e64):
    S0, K, _, _, _, _, W, _, M, _, _ = scalars(run)
    return path_bar(np.array(e64), magnitudes(S0, K, W, M))


def err(got, want):
    """|float − mpf| without rounding the exact value first"""
    with mp.workdps(DPS):
        return float(abs(mp.mpf(float(got)) - want))
