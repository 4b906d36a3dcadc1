"""Writes tests/golden/qe_exact.json: the fixtures of the quadratic-exponential tests (tests/qe_cases.py).  CPU only.

  branches  per model and n_steps of the device tests, on their fixed seeds, mirrors included: how many member-steps
            take the quadratic branch, the exponential branch, and its U <= p arm.  The walk asserts on EVERY trajectory
            that the fp64 run and the 50-digit run take the same branches and that |ψ − ψ_c| and |U − p| exceed
            qe_cases.MARGIN at every step — none is left out; a seed set that fails is changed, not the rule.  On more
            than one step all three counts must be positive for either model; on one step every member starts at V0 and
            so shares one ψ: "feller" is then quadratic, "low_v0" exponential with both arms of U.
  rows      the 50-digit statistics (five rows and var_T, 30 digits) of the first GOLDEN_N trajectories and their
            mirrors at GOLDEN_SHAPE, with and without the correction, and their bars 20·max(e64, ε·A): what the mutation
            tests of tests/test_qe_host.py hold a mutated restatement to.

Run from the repository root:  python tests/golden/make_qe_exact.py
"""
import json
import os
import sys

import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import euler_tangent_cases as etc  # noqa: E402
from tests import oracle_ffi  # noqa: E402
from tests import qe_cases as qc  # noqa: E402


def build(oracle):
    seeds = qc.path_seeds()
    branches, rows = [], []
    for n_steps in sorted({s for s, _ in qc.PATH_SHAPES}):
        Z = qc.step_normals(oracle, seeds, n_steps)
        U = qc.step_uniforms(oracle, seeds, n_steps)
        for name, case in qc.MODELS.items():
            runs, counts = qc.walks(case, n_steps, Z, U, anti=1, mart=0, check=True)
            if n_steps > 1:
                assert all(counts[k] > 0 for k in counts), (name, n_steps, counts)
            elif name == "feller":
                assert counts["exponential"] == 0 and counts["quadratic"] > 0, counts
            else:
                assert counts["quadratic"] == 0 and 0 < counts["zero"] < counts["exponential"], counts
            branches.append(dict(model=name, n_steps=n_steps, **counts))
            if n_steps != qc.GOLDEN_SHAPE[0]:
                continue
            for mart in (0, 1):
                runs, _ = qc.walks(case, n_steps, Z, U, anti=1, mart=mart, n=qc.GOLDEN_N)
                ref = qc.reference(case, runs, qc.GOLDEN_SHAPE[1], 0)
                bars = etc.path_bar(ref["e64"], ref["A"])
                with mp.workdps(qc.DPS):
                    want = [[[mp.nstr(t, 30) for t in ref["want"][m][i]] for i in range(qc.GOLDEN_N)] for m in range(2)]
                rows.append(dict(model=name, martingale=mart, want=want, bars=[[list(map(float, b)) for b in bm] for bm in bars]))
    return dict(note="written by tests/golden/make_qe_exact.py; see its docstring", margin=qc.MARGIN,
                n_paths=qc.PATH_N, golden_n=qc.GOLDEN_N, golden_shape=list(qc.GOLDEN_SHAPE), branches=branches, rows=rows)


def main():
    doc = build(oracle_ffi.load())
    with open(qc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(qc.GOLDEN, os.path.getsize(qc.GOLDEN), "bytes")
    for b in doc["branches"]:
        print(b)


if __name__ == "__main__":
    main()
