"""Writes tests/golden/localvol_exact.json and, beside it, the two float64 arrays it describes (localvol_exact_coarse.npy,
localvol_exact_fine.npy): CEV call prices (Schroder's closed form, tests/localvol_cases.cev_call, at 30 digits and rounded
once to fp64) on the Dupire stencils of two grids, the second with dk and dT halved.

  model   dS = rS dt + δ S^β dW,  S0 = 100, r = 0.03, β = 0.5, δ = 0.25·S0^{0.5}: σ(S) = 0.25·(S/S0)^{−0.5}
  grid    21 times 0.05, 0.10, …, 1.05 × 257 nodes over log S0 ± 1.5
  stencil per node (T, k = log K): C(T, k), C(T, k + dk), C(T, k − dk), C(T + dT, k), C(T − dT, k)
  coarse  dk = 0.02, dT = 0.01, recorded at the CENTRE nodes alone — |x − log S0| <= 2.5·0.25·√t, where the convergence
          test reads it: the JSON lists the nodes [j, i], the array holds their five prices, [n_centre][5]
  fine    dk = 0.01, dT = 0.005, every node: prices[5][21][257] (the device test makes its Dupire table from it)

Run from the repository root:  python tests/golden/make_localvol_exact.py   (a few minutes on several cores)."""
import json
import math
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import localvol_cases as lc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "localvol_exact.json")
N_T, N_X, HALF_WIDTH = 21, 257, 1.5
GRIDS = {"coarse": (0.02, 0.01), "fine": (0.01, 0.005)}
DIGITS = 30


def nodes():
    x0 = math.log(lc.CEV["S0"])
    h = 2 * HALF_WIDTH / (N_X - 1)
    return [0.05 * (j + 1) for j in range(N_T)], [x0 - HALF_WIDTH + h * i for i in range(N_X)]


def centre(t, x):
    return abs(x - math.log(lc.CEV["S0"])) <= 2.5 * lc.CEV["sigma0"] * math.sqrt(t)


def stencil(t, x, dk, dT):
    return [(t, x), (t, x + dk), (t, x - dk), (t + dT, x), (t - dT, x)]


def price(tk):
    with mp.workdps(DIGITS):
        return float(lc.cev_call(tk[0], mp.exp(mp.mpf(tk[1]))))


def main():
    times, xs = nodes()
    jobs, where = [], []
    for name, (dk, dT) in GRIDS.items():
        for j, t in enumerate(times):
            for i, x in enumerate(xs):
                if name == "fine" or centre(t, x):
                    for s, tk in enumerate(stencil(t, x, dk, dT)):
                        jobs.append(tk)
                        where.append((name, j, i, s))
    with Pool(min(os.cpu_count() or 1, 16)) as pool:
        got = pool.map(price, jobs, chunksize=64)
    fine = [[[None] * N_X for _ in range(N_T)] for _ in range(5)]
    coarse = {}
    for (name, j, i, s), c in zip(where, got):
        if name == "fine":
            fine[s][j][i] = c
        else:
            coarse.setdefault((j, i), [None] * 5)[s] = c
    centre_nodes = sorted(coarse)
    doc = dict(model=lc.CEV, digits=DIGITS, times=times, x_lo=xs[0], x_hi=xs[-1], n_x=N_X,
               grids={k: dict(dk=v[0], dT=v[1]) for k, v in GRIDS.items()},
               coarse_nodes=[list(k) for k in centre_nodes], coarse="localvol_exact_coarse.npy [n_centre][5]",
               fine="localvol_exact_fine.npy [5][n_times][n_x]")
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    np.save(OUT.replace(".json", "_coarse.npy"), np.array([coarse[k] for k in centre_nodes], dtype=np.float64))
    np.save(OUT.replace(".json", "_fine.npy"), np.array(fine, dtype=np.float64))
    print(OUT, os.path.getsize(OUT), "bytes;", len(jobs), "prices")


if __name__ == "__main__":
    main()
