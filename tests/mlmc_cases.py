"""Multilevel Monte Carlo: the cases of tests/test_gpu_mlmc.py and tests/test_mlmc_host.py, and a numpy restatement of the
coupled levels — HestonModel<0, true>'s step (csrc/hh_sim.h) on numpy's own normals, a fine and a coarse trajectory per
column on the same increments, the coarse increment the sum of the fine pair's — whose per-level means and variances
tests/golden/mlmc_exact.json records (tests/golden/make_mlmc_exact.py writes it).  The restatement shares no draw with the
device: it says what the coupling is worth in this model at the tests' sizes, which is what the device tests' conditions
are set from."""
import json
import math
import os

import numpy as np

from tests import path_payoff_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlmc_exact.json")

# the mild case: the Feller condition holds (2·κ·θ = 0.12 > σ² = 0.09)
MILD = dict(S0=100.0, K=100.0, V0=0.04, kappa=1.5, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0)
STEPS0, DATES = 4, 4            # level 0 runs 4 steps; the Asian averages over 4 dates, one per level-0 step
TRAJECTORIES = (2 ** 18, 2 ** 16, 2 ** 15, 2 ** 14)  # per level (steps 4, 8, 16, 32), on the device and in the restatement alike
RESTATED_SEEDS = (1, 2)
PAYOFFS = {"call": pc.payoff(pc.VANILLA, MILD["K"], 1.0), "asian": pc.payoff(pc.ARITH, MILD["K"], 1.0)}
# the conditions of the coupling test, and the margin the restatement must keep on each
V1_OVER_VAR0, DECAY, MARGIN = 1.0 / 4.0, 0.7, 1.25


def heston_step(x, v, dt, dW1, dW2, p=MILD):
    """one split-step Euler–Maruyama step on (log S, V): drift first, diffusion at the drift-updated clipped variance"""
    vp = np.maximum(v, 0.0)
    Kx = x + dt * (p["r"] - 0.5 * vp)
    Kv = v + dt * (p["kappa"] * (p["theta"] - vp))
    sq = np.sqrt(np.maximum(Kv, 0.0))
    return Kx + sq * dW1, Kv + (p["sigma"] * sq) * dW2


def running_stats(n):
    return dict(first=True, st=np.zeros((pc.S_T + 1, n)))


def take_date(run, x):
    S, st = np.exp(x), run["st"]
    if run["first"]:
        st[pc.SUM_S], st[pc.SUM_X], st[pc.MAX_S], st[pc.MIN_S] = S, x, S, S
        run["first"] = False
    else:
        st[pc.SUM_S] += S
        st[pc.SUM_X] += x
        st[pc.MAX_S] = np.maximum(st[pc.MAX_S], S)
        st[pc.MIN_S] = np.minimum(st[pc.MIN_S], S)
    st[pc.S_T] = S


def coupled_stats(rng, n, n_fine, every, p=MILD):
    """(fine statistics, coarse statistics), each (5, n): n_fine fine steps monitored every `every` of them, n_fine/2 coarse
    steps on the summed increments monitored every `every`/2"""
    assert n_fine % 2 == 0 and every % 2 == 0 and n_fine % every == 0
    dt, rho_c = p["T"] / n_fine, math.sqrt(1.0 - p["rho"] ** 2)
    dtc = p["T"] / (n_fine // 2)
    xf = np.full(n, math.log(p["S0"]))
    vf = np.full(n, p["V0"])
    xc, vc = xf.copy(), vf.copy()
    fine, coarse = running_stats(n), running_stats(n)
    for j in range(n_fine // 2):
        s1 = s2 = 0.0
        for h in range(2):
            z1, z2 = rng.standard_normal(n), rng.standard_normal(n)
            d1, d2 = math.sqrt(dt) * z1, math.sqrt(dt) * (p["rho"] * z1 + rho_c * z2)
            xf, vf = heston_step(xf, vf, dt, d1, d2, p)
            if (2 * j + h + 1) % every == 0:
                take_date(fine, xf)
            s1, s2 = s1 + d1, s2 + d2
        xc, vc = heston_step(xc, vc, dtc, s1, s2, p)
        if (j + 1) % (every // 2) == 0:
            take_date(coarse, xc)
    return fine["st"], coarse["st"]


def plain_stats(rng, n, n_steps, every, p=MILD):
    """level 0: the statistics of n_steps plain steps"""
    dt, rho_c = p["T"] / n_steps, math.sqrt(1.0 - p["rho"] ** 2)
    x, v, run = np.full(n, math.log(p["S0"])), np.full(n, p["V0"]), running_stats(n)
    for s in range(n_steps):
        z1, z2 = rng.standard_normal(n), rng.standard_normal(n)
        x, v = heston_step(x, v, dt, math.sqrt(dt) * z1, math.sqrt(dt) * (p["rho"] * z1 + rho_c * z2), p)
        if (s + 1) % every == 0:
            take_date(run, x)
    return run["st"]


def every_of(name, level):
    """monitor_every of a payoff on level l: the Asian's dates are the level-0 steps, the call looks at expiry alone"""
    return (1 if name == "asian" else STEPS0) << level


def restate(seed, counts=TRAJECTORIES):
    """{payoff: {"mean": [m_0 … m_{L}], "var": [Var P_0, V_1 … V_L]}}, undiscounted, counts[l] trajectories on level l"""
    out = {}
    for k, (name, q) in enumerate(PAYOFFS.items()):
        rng = np.random.default_rng([seed, k])
        nm = DATES if name == "asian" else 1
        y = pc.payoff_from_stats(plain_stats(rng, counts[0], STEPS0, every_of(name, 0)), q, nm)
        mean, var = [float(y.mean())], [float(y.var(ddof=1))]
        for level in range(1, len(counts)):
            f, c = coupled_stats(rng, counts[level], STEPS0 << level, every_of(name, level))
            y = pc.payoff_from_stats(f, q, nm) - pc.payoff_from_stats(c, q, nm)
            mean.append(float(y.mean()))
            var.append(float(y.var(ddof=1)))
        out[name] = dict(mean=mean, var=var)
    return out


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)
