"""Writes tests/golden/merton_exact.json: the fixtures of the Merton tests (tests/merton_cases.py).

  poisson     (U, m) pairs for m = 0, 1e-3, 1, 8, 64 with the jump count of the exact (50-digit) inversion; every U
              keeps merton_cases.MARGIN from every exact cumulative boundary, so the 1e-16 of the fp64 sums cannot move
              the count.  `edges`: U = 2⁻⁵³ and U = 1 − 2⁻⁵³ at every m and at m = 2.5, where the fp64 cumulative sum
              saturates below the largest uniform and the cap decides; recorded with the count of the fp64 loop.
  carr_madan  baskets for hh_carr_madan_jump: per payoff the exactly integrated truncated integral (30 digits) and e64,
              the distance of the fp64 numpy restatement of the device's rule from it.
  counts      the jump counts of the device tests' fixed seeds, by the exact inversion on the uniforms of the oracle's
              host Philox; the margin is asserted on every one, and each path shape must show N = 0, 1 and >= 2.
  series      the worked example of the header: Merton's series at 30 digits.

Run from the repository root:  python tests/golden/make_merton_exact.py
"""
import json
import math
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import merton_cases as mc  # noqa: E402
from tests import oracle_ffi  # noqa: E402

POISSON_MEANS = (0.0, 1e-3, 1.0, 8.0, 64.0)
EDGE_MEANS = POISSON_MEANS + (2.5,)
PER_MEAN = 24


def poisson_fixtures():
    rng = np.random.default_rng(20261019)
    out = []
    for m in POISSON_MEANS:
        us, ns = [], []
        while len(us) < PER_MEAN:
            # the device's uniforms: (k + ½)·2⁻⁵², k of 52 bits — half of them from the tails, where large counts live
            k = int(rng.integers(0, 2**52))
            if len(us) % 2:
                k = 2**52 - 1 - (k >> int(rng.integers(8, 40)))
            u = mc.uniform_of(k)
            n, dist = mc.poisson_exact(u, m)
            if dist < mc.MARGIN and m > 0.0:
                continue
            us.append(u.hex())
            ns.append(n)
        out.append(dict(m=float(m).hex(), U=us, N=ns))
    edges = [dict(U=u.hex(), m=float(m).hex(), N=mc.poisson_fp64(u, m))
             for m in EDGE_MEANS for u in (2.0 ** -53, 1.0 - 2.0 ** -53)]
    return out, edges


def cm_baskets():
    """name -> (model, alpha, bound, [(K, cp, T)])"""
    strikes = [70.0 + 60.0 * k / 32 for k in range(33)]
    return {
        "single": (mc.BASE, 1.0, 20.0, [(105.0, 1.0, 1.0)]),
        "basket33": (mc.BASE, 1.5, 24.0, [(K, 1.0 if k % 3 else -1.0, 0.5 if k % 2 else 1.5) for k, K in enumerate(strikes)]),
        "lambda0": (dict(mc.BASE, lam=0.0), 1.0, 20.0, [(90.0, 1.0, 1.0), (105.0, -1.0, 1.0), (120.0, 1.0, 0.5)]),
    }


def carr_madan_fixtures():
    out = []
    for name, (model, alpha, bound, payoffs) in cm_baskets().items():
        rows = []
        for K, cp, T in payoffs:
            case = cl.cm_case(dict(model, T=T), K, alpha, bound, cp)
            call = cl.cm_exact_call(case, mc.log_cf)
            with mp.workdps(mc.DPS):
                price = call if cp > 0 else call + cl.cm_parity(case)
                rows.append(dict(K=K, cp=cp, T=T, price=mp.nstr(price, 30), e64=cl.cm_e64(case, call, mc.phi)))
        out.append(dict(id=name, model={k: float(v) for k, v in model.items()}, alpha=alpha, bound=bound, payoffs=rows))
    return out


def count_fixtures(oracle):
    terminal = []
    for off in mc.TERMINAL_OFFSETS:
        U = mc.terminal_uniforms(oracle, mc.TERMINAL_SEED, off, mc.TERMINAL_N)
        for mean in mc.TERMINAL_MEANS:
            if mean > 0.0:
                N = mc.counts_of(U, mc.terminal_case(mean, 0)["lam"] * mc.BASE["T"])
                assert N.max() <= mc.MAX_COUNT
                terminal.append(dict(path_offset=off, mean=mean, N=[int(t) for t in N]))
    path = []
    for n_steps in sorted({s for s, _ in mc.PATH_SHAPES}):
        U = mc.path_uniforms(oracle, mc.path_seeds(), n_steps)
        N = mc.counts_of(U, mc.path_mean(mc.path_case(n_steps, 0)))
        assert (N == 0).any() and (N == 1).any() and (N >= 2).any(), n_steps
        path.append(dict(n_steps=n_steps, N=[[int(t) for t in row] for row in N]))
    return dict(terminal=terminal, path=path)


def build(oracle):
    poisson, edges = poisson_fixtures()
    return dict(note="written by tests/golden/make_merton_exact.py; see its docstring", margin=mc.MARGIN,
                poisson=poisson, edges=edges, carr_madan=carr_madan_fixtures(), counts=count_fixtures(oracle),
                series=dict(model=mc.BASE, K=105.0, cp=1.0, price=mp.nstr(mc.series(mc.BASE, 105.0, 1.0), 30)))


def main():
    doc = build(oracle_ffi.load())
    with open(mc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
