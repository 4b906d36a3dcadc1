"""Writes tests/golden/lognormal_exact.json: the inputs of the lognormal exact-law cases and a digest of their 50-digit
reference (oracle/lognormal_exact.py).  Run from the repository root: python tests/golden/make_lognormal_exact.py

The file holds inputs only — model scalars, the two flags, payoffs, and ONE block of 32 standard normals as INTEGERS k
with z = k·2⁻⁴⁰, so that every machine forms the same doubles — and per payoff the 50-digit sum over the paths of the
price contribution and its eight partials, as 30-digit strings, by which tests/test_lognormal_exact_host.py notices
drift of the reference module.  The per-path reference itself is cheap and is recomputed by the tests.

The 32 normals: 26 draws of numpy's generator interleaved with 0.0, −0.0, ±8.5 and two values below 2⁻³⁰.  The draws'
seed is the first one with which the reference alone leaves out no path of any case (no payoff comparison within
2⁻³⁰·A of a tie, fp64 on the same side); the host test asserts that again on the committed file.
"""
import json
import math
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import lognormal_exact as lx  # noqa: E402
from tests import lognormal_exact_cases as lc  # noqa: E402

SCALE = 2 ** 40


def model(S0=100.0, sigma=0.2, r=0.05, T=1.0):
    return dict(S0=S0, sigma=sigma, r_drift=r, T=T, discount=math.exp(-r * T))


# tag -> (model, strikes)
MODELS = {
    "ref": (model(S0=1.0, sigma=1.0, r=0.03, T=366 / 365), [1.0]),   # the reference's Greeks scenario
    "bench": (model(), [50.0, 100.0, 300.0]),                         # config 2; deep in and deep out of the money
    "tiny-sigma": (model(sigma=1e-8), [100.0]),                       # σ·√T·z underflows against the mean
    "sigma0": (model(sigma=0.0), [100.0]),                            # every sample equal: S0·e^{r·m} = 105.1, off the strike
    "short": (model(r=-0.01, T=1 / 365), [100.0]),                    # √T = 0.052 against T = 0.0027
    "scale-small": (model(S0=1e-3), [1e-3]),                          # log S0 = −6.9
    "scale-large": (model(S0=1e6), [1e6]),                            # log S0 = +13.8
}
# positions of the special normals among the 32; the other 26 are drawn
SPECIAL = {1: 0, 3: "-0", 4: int(8.5 * SCALE), 6: -int(8.5 * SCALE), 7: 513, 9: -1}


def records():
    out = []
    for tag, (m, strikes) in MODELS.items():
        for compat in (0, 1):
            for anti in (0, 1):
                out.append(dict(id=f"{tag}{'-compat' if compat else ''}{'-anti' if anti else ''}", tag=tag, model=m,
                                compat_sqrt_alpha=compat, antithetic=anti,
                                payoffs=[dict(strike=K, cp=cp) for cp in (1.0, -1.0) for K in strikes]))
    return out


def draw(seed):
    rng = np.random.default_rng(seed)
    k, neg_zero = [], []
    for i in range(32):
        s = SPECIAL.get(i)
        if s is None:
            k.append(int(np.rint(rng.standard_normal() * SCALE)))
        else:
            k.append(0 if s == "-0" else s)
            if s == "-0":
                neg_zero.append(i)
    return dict(k=k, neg_zero=neg_zero)


def digest(ref, pj):
    paths = lc.usable_paths(ref, ref["payoffs"].index(pj))
    with mp.workdps(lx.DPS):
        return [mp.nstr(mp.fsum(pj["price"][i][s] for i in paths), 30) for s in range(1 + lx.NS)]


def main():
    for seed in range(1, 50):
        recs = records()
        doc = dict(slots=list(lx.SLOTS), scale=SCALE, draw_seed=seed, normals=draw(seed), cases=recs)
        z = lc.normals_of(doc)
        left_out = 0
        for r in recs:
            case = lc.expand(r, z)
            ref = lx.reference(case, case["payoff_list"])
            for p, pj in zip(r["payoffs"], ref["payoffs"]):
                left_out += int((~pj["usable"]).sum())
                p["price_sum"] = digest(ref, pj)
        if left_out == 0:
            break
        print(f"seed {seed}: {left_out} paths left out")
    else:
        raise SystemExit("no seed meets the condition")
    with open(lc.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"seed {seed}: wrote {lc.GOLDEN}, {os.path.getsize(lc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
