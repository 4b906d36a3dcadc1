"""Writes tests/golden/vg_exact.json: the fixtures of the Variance Gamma tests (tests/vg_cases.py).

  sampler     per shape (0.008, 0.25, 1, 4.7, 1e4) samples of csrc/hh_vg.h's gamma_mt: the draws of every attempt up to the
              accepted one (z from a normal twice as wide as the standard one and, in every other sample, a first U
              close to 1, so that rejections and proposals with v <= 0 are frequent), the number of attempts, the variate
              of the 50-digit restatement (30 digits), its bar and the smallest decision margin met.  Only attempts whose margins |rhs − log U| and |1 + c·z| are at least
              vg_cases.MARGIN are kept — asserted — so the 1e-15 of the fp64 sums cannot move a decision.
  prices      the gamma-mixing integral at 30 digits for the three parameter sets, K = 80, 100, 120, calls and puts.
  carr_madan  per parameter set a basket for hh_carr_madan_vg: per payoff the exactly integrated truncated integral and
              e64, the distance of the fp64 numpy restatement of the device's rule from it; `tail`: a basket at a bound
              where the bound on what the truncation leaves out (vg_cases.cm_tail_bound) is below 1e-10·S0 — asserted.
  counts      the attempts of every variate the device tests draw on their fixed seeds, by the 50-digit walk on the
              oracle's host Philox; the margin is asserted on every attempt.

Run from the repository root:  python tests/golden/make_vg_exact.py
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import oracle_ffi  # noqa: E402
from tests import vg_cases as vc  # noqa: E402

PER_SHAPE = 32
SAMPLER_NU = 0.5      # span = shape·0.5 exactly (a power of two): span/ν is the shape, bit for bit
CM_ALPHA, CM_BOUND = 1.5, 32.0
TAIL_BOUND = 200.0    # on the third parameter set, T/ν = 10: the integrand decays like v^−22


def sampler_fixtures():
    rng = np.random.default_rng(20261021)
    out = []
    for shape in vc.HOST_SHAPES:
        span = shape * SAMPLER_NU
        assert span / SAMPLER_NU == shape
        with mp.workdps(vc.DPS):
            g50 = vc.vg_args(mp.mpf, 0.0, 0.0, 0.0, SAMPLER_NU, span)
            g64 = vc.vg_args(float, 0.0, 0.0, 0.0, SAMPLER_NU, span)
            assert g50["boost"] == (shape < 1.0)
            samples = []
            while len(samples) < PER_SHAPE:
                draws = []
                while True:  # one attempt after the other, each kept only with its margin, until one is accepted
                    z = float(2.0 * rng.standard_normal())
                    U, Ub = vc.u01(int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))), \
                        vc.u01(int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)))
                    if len(samples) % 2 and not draws:  # every other sample: a first U from the top, where rhs < 0 rejects
                        U = 1.0 - U * 2.0 ** -int(rng.integers(8, 40))
                    try:
                        _, n, margin = vc.gamma_walk(g50, [(mp.mpf(t[0]), t[1], t[2]) for t in draws] + [(mp.mpf(z), U, Ub)], mp.mpf)
                        accepted = True
                    except ValueError:  # rejected: the walk asks for the next attempt
                        accepted = False
                        _, _, margin = vc.gamma_walk(g50, [(mp.mpf(z), U, Ub)] * vc.MAX_ATTEMPTS, mp.mpf)
                    if margin < vc.MARGIN:
                        continue
                    draws.append((z, U, Ub))
                    if accepted:
                        break
                r = vc.variate_reference(g50, g64, [(mp.mpf(z), U, Ub) for z, U, Ub in draws])
                assert r["attempts"] == len(draws) and r["margin"] >= vc.MARGIN
                samples.append(dict(draws=[[float(z).hex(), float(U).hex(), float(Ub).hex()] for z, U, Ub in draws],
                                    attempts=r["attempts"], variate=mp.nstr(r["want"], 30), bar=r["bar"], margin=r["margin"]))
        assert any(s["attempts"] >= 2 for s in samples), shape
        out.append(dict(shape=shape, span=float(span).hex(), nu=float(SAMPLER_NU).hex(), samples=samples))
    return out


def price_fixtures():
    out = []
    for p in vc.PARAMS:
        case = vc.params_case(p)
        for K in vc.STRIKES:
            for cp in (1.0, -1.0):
                out.append(dict(params=list(p), K=K, cp=cp, price=mp.nstr(vc.mixing_price(case, K, cp), 30)))
    return out


def _cm_rows(case, alpha, bound):
    rows = []
    for K in vc.STRIKES:
        cmc = cl.cm_case(case, K, alpha, bound)
        call = cl.cm_exact_call(cmc, vc.log_cf)
        e64 = cl.cm_e64(cmc, call, vc.phi)
        for cp in (1.0, -1.0):
            with mp.workdps(vc.DPS):
                price = call if cp > 0 else call + cl.cm_parity(cmc)
                rows.append(dict(K=K, cp=cp, T=case["T"], price=mp.nstr(price, 30), e64=e64))
    return rows


def carr_madan_fixtures():
    out = []
    for i, p in enumerate(vc.PARAMS):
        case = vc.params_case(p)
        out.append(dict(id=f"set{i}", model={k: float(v) for k, v in case.items()}, alpha=CM_ALPHA, bound=CM_BOUND,
                        payoffs=_cm_rows(case, CM_ALPHA, CM_BOUND)))
    case = vc.params_case(vc.PARAMS[2])
    tails = [float(vc.cm_tail_bound(cl.cm_case(case, K, CM_ALPHA, TAIL_BOUND))) for K in vc.STRIKES]
    assert max(tails) < 1e-10 * case["S0"], tails
    tail = dict(id="tail", model={k: float(v) for k, v in case.items()}, alpha=CM_ALPHA, bound=TAIL_BOUND, tail=max(tails),
                payoffs=_cm_rows(case, CM_ALPHA, TAIL_BOUND))
    for row in tail["payoffs"]:
        row["mixing"] = mp.nstr(vc.mixing_price(case, row["K"], row["cp"]), 30)
    return out + [tail]


def count_fixtures(oracle):
    terminal, path = [], []
    seeds = vc.path_seeds()
    for shape in vc.DEVICE_SHAPES:
        d = vc.PathDraws(oracle, vc.shape_case(shape, 1), 1, vc.PATH_N, [vc.TERMINAL_SEED], terminal=True)
        assert d.margin >= vc.MARGIN, (shape, d.margin)
        terminal.append(dict(shape=shape, attempts=[a[0] for a in d.attempts]))
        for n_steps in vc.PATH_STEPS:
            d = vc.PathDraws(oracle, vc.shape_case(shape, n_steps), n_steps, vc.PATH_N, seeds)
            assert d.margin >= vc.MARGIN, (shape, n_steps, d.margin)
            path.append(dict(shape=shape, n_steps=n_steps, attempts=d.attempts))
    return dict(terminal=terminal, path=path)


def build(oracle, counts=True):
    doc = dict(note="written by tests/golden/make_vg_exact.py; see its docstring", margin=vc.MARGIN,
               sampler=sampler_fixtures(), prices=price_fixtures(), carr_madan=carr_madan_fixtures())
    if counts:
        doc["counts"] = count_fixtures(oracle)
    return doc


def main():
    doc = build(oracle_ffi.load())
    with open(vc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(vc.GOLDEN, os.path.getsize(vc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
