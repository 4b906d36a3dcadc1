"""Writes tests/golden/sobol_exact.json: what the numpy restatement of tests/sobol_cases.py — the library's own points and
shift rule, scipy's quantile, the split-step Euler scheme in numpy — gives for the convergence conditions of
tests/test_gpu_sobol.py on their fixed seed, so that a reader sees the margin each condition has.  Run on the CPU.

  (c) Heston Euler, 16 steps, N = 2^14, R = 16, bridge: the RQMC standard error over the standard error of a
      pseudo-random solve of the same budget 16·N must be at most 0.5; the seed is kept only if the restatement's ratio is
      at most 0.5 / 1.25.
  (d) 64 steps: the bridge's standard error must be below the incremental one; kept only if it is below by 1.25x.
The pseudo-random standard error is sd(payoff)/sqrt(16·N) with the payoff's standard deviation taken from the
restatement's own 16·N quasi-random payoffs: the law's, whatever the points.

    python tests/golden/make_sobol_exact.py
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import sobol_cases as sc  # noqa: E402


def heston_rqmc(n_steps, construction, seed=sc.CONV_SEED, n=sc.CONV_N_HESTON, R=sc.CONV_R):
    """(estimates [R], standard deviation of one discounted payoff)"""
    est, var = [], []
    for r in range(R):
        z = sc.normals_np(n_steps, 2, n, r, seed)
        pay = sc.heston_euler_payoffs(sc.HESTON, n_steps, sc.steps_np(n_steps, construction, z[0::2]),
                                      sc.steps_np(n_steps, construction, z[1::2]))
        est.append(float(pay.mean()))
        var.append(float(pay.var(ddof=1)))
    return est, math.sqrt(float(np.mean(var)))


def build():
    doc = {"seed": sc.CONV_SEED, "points": sc.CONV_N_HESTON, "randomizations": sc.CONV_R, "margin": sc.CONV_MARGIN,
           "model": sc.HESTON}
    est, sd = heston_rqmc(16, sc.BRIDGE)
    mean, se = sc.rqmc(est)
    se_mc = sd / math.sqrt(sc.CONV_R * sc.CONV_N_HESTON)
    doc["steps16"] = {"price": mean, "std_error": se, "pseudo_random_std_error": se_mc, "ratio": se / se_mc}
    assert se / se_mc <= 0.5 / sc.CONV_MARGIN, doc["steps16"]
    se64 = {name: sc.rqmc(heston_rqmc(64, c)[0])[1] for name, c in (("bridge", sc.BRIDGE), ("incremental", sc.INCREMENTAL))}
    doc["steps64"] = dict(se64, ratio=se64["bridge"] / se64["incremental"])
    assert se64["bridge"] * sc.CONV_MARGIN <= se64["incremental"], doc["steps64"]
    return doc


if __name__ == "__main__":
    with open(sc.GOLDEN, "w") as f:
        json.dump(build(), f, indent=1)
        f.write("\n")
    print(open(sc.GOLDEN).read())
