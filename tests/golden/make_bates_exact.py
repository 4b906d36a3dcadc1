"""Writes tests/golden/bates_exact.json: the fixtures of the Bates tests (tests/bates_cases.py).  CPU only.

  seen      per model and n_steps of the device tests, on their fixed seeds, mirrors included: how many member-steps take
            the quadratic branch, the exponential branch and its U <= p arm, and how many saw each jump count N.  The
            walk asserts on EVERY trajectory that the fp64 run and the 50-digit run take the same QE branches with
            |ψ − ψ_c| and |U − p| above qe_cases.MARGIN, and merton_cases.counts_of asserts that every jump uniform keeps
            merton_cases.MARGIN from every exact cumulative boundary and that the fp64 search finds the exact count —
            none is left out; a seed set that fails is changed, not the rule.  On more than one step a case must see
            both QE branches and an N >= 2; the one-step shape is exempt (every member starts at V0 and shares one ψ).
  rows      the 50-digit statistics (five rows and var_T, 30 digits) of the first GOLDEN_N trajectories and their
            mirrors at GOLDEN_SHAPE, with and without the correction, and their bars 20·max(e64, ε·A): what the mutation
            tests of tests/test_bates_host.py hold a mutated restatement to.
  carr_madan  the exactly integrated truncated Carr–Madan calls of bates_cases.cm_cases() (30 digits) and the fp64
            rounding e64 of the rule on each.

Run from the repository root:  python tests/golden/make_bates_exact.py
"""
import json
import os
import sys

import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bates_cases as bt  # noqa: E402
from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import oracle_ffi  # noqa: E402


def build(oracle):
    seeds = bt.path_seeds()
    seen, rows = [], []
    for n_steps in sorted({s for s, _ in bt.PATH_SHAPES}):
        d = bt.draws(oracle, seeds, n_steps)
        for name in bt.MODELS:
            case = bt.path_case(name, n_steps)
            N = bt.counts(d["UJ"], bt.path_mean(case, n_steps))
            _, saw = bt.walks(case, n_steps, d, N, anti=1, mart=0, check=True)
            if n_steps > 1:
                assert saw["quadratic"] > 0 and saw["exponential"] > 0 and max(saw["N"]) >= 2, (name, n_steps, saw)
            seen.append(dict(model=name, n_steps=n_steps, quadratic=saw["quadratic"], exponential=saw["exponential"],
                             zero=saw["zero"], N={str(k): v for k, v in sorted(saw["N"].items())}))
            if n_steps != bt.GOLDEN_SHAPE[0]:
                continue
            for mart in (0, 1):
                runs, _ = bt.walks(case, n_steps, d, N, anti=1, mart=mart, n=bt.GOLDEN_N)
                ref = bt.reference(case, runs, bt.GOLDEN_SHAPE[1], 0)
                bars = etc.path_bar(ref["e64"], ref["A"])
                with mp.workdps(bt.DPS):
                    want = [[[mp.nstr(t, 30) for t in ref["want"][m][i]] for i in range(bt.GOLDEN_N)] for m in range(2)]
                rows.append(dict(model=name, martingale=mart, want=want, bars=[[list(map(float, b)) for b in bm] for bm in bars]))
    cm = {}
    for key, case in bt.cm_cases().items():
        exact = cl.cm_exact_call(case, bt.log_cf)
        with mp.workdps(bt.DPS):
            cm[key] = dict(call=mp.nstr(exact, 30), e64=cl.cm_e64(case, exact, bt.phi))
    return dict(note="written by tests/golden/make_bates_exact.py; see its docstring", margin=bt.qc.MARGIN,
                n_paths=bt.PATH_N, golden_n=bt.GOLDEN_N, golden_shape=list(bt.GOLDEN_SHAPE), seen=seen, rows=rows, carr_madan=cm)


def main():
    doc = build(oracle_ffi.load())
    with open(bt.GOLDEN, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(bt.GOLDEN, os.path.getsize(bt.GOLDEN), "bytes")
    for b in doc["seen"]:
        print(b)
    for k, v in doc["carr_madan"].items():
        print(k, v)


if __name__ == "__main__":
    main()
