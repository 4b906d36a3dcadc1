"""Writes tests/golden/path_sweep.json: the fixture of the sweep over model values (tests/path_sweep_cases.py).  CPU only.

  drawn   per family, the first DRAWN_N models of path_sweep_cases.draw_models whose share of unusable trajectories is
          within the cap, as hex floats: every machine forms the same doubles.  A draw that breaks the cap is passed over
          for the next of the same stream; the rule is never relaxed.
  cases   per case — edge rows and drawn models — and per shape: the counts that show what the case exercised (QE branch
          counts, the jump-count histogram, K3, E, 1 − E, A, trajectories left out), and per (shape, include_start) a
          30-digit digest of the 50-digit reference: the sum over the usable members, mirrors included, of each row.
          The host test notices a drift of a restatement through it.
Before it writes, the script asserts path_sweep_cases.check_expectations on every case: a ψ_c case sees both branches, a
mean-64 case some N >= 40, a ρ = ±1 case has K3 == 0.0 exactly, no case leaves out more than one trajectory of 65.  It
stores inputs, counts and digests, not per-path rows, one record per line so that a changed digest shows in a diff.

Run from the repository root:  python tests/golden/make_path_sweep.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import oracle_ffi  # noqa: E402
from tests import path_sweep_cases as sw  # noqa: E402


def record(oracle, case):
    """-> the fixture's record of a case, or None when it breaks the unusable cap"""
    walks = {key: sw.walk(oracle, case, key) for key, _ in sw.shapes_of(case)}
    if any(w["counts"]["unusable"] > sw.CAP for w in walks.values()):
        return None
    sw.check_expectations(case, walks)
    rec = dict(id=sw.case_id(case), digests={})
    for key, every, start in sw.combos(case):
        ref = sw.reference(case, walks[key], every, start)
        rec["digests"][f"{key}x{every}+{start}"] = sw.digest(ref, walks[key]["usable"])
    sw.check_expectations(case, walks)   # again: local volatility counts its off-grid states in the reference
    rec["counts"] = {str(k): sw.json_counts(w["counts"]) for k, w in walks.items()}
    return rec


def build(oracle):
    drawn, cases = {}, []
    for family in sw.FAMILIES:
        for case in sw.EDGE[family]:
            for n_steps, _ in (sw.SHAPES if family != "merton_terminal" else ((1, 1),)):
                assert sw.defect(case, n_steps) is None, (sw.case_id(case), n_steps, sw.defect(case, n_steps))
            rec = record(oracle, case)
            assert rec is not None, f"{sw.case_id(case)} breaks the unusable cap: give the row another value of its kind"
            cases.append(rec)
        for _, case, n_steps, code, text in sw.rejected(family):
            got = sw.defect(case, n_steps)
            assert got == (code, text), (case, got)
        keep, passed = [], []
        for case in sw.draw_models(family):
            rec = record(oracle, case)
            if rec is None:
                passed.append(case["name"])
                continue
            keep.append(sw.to_hex(case))
            cases.append(rec)
            if len(keep) == sw.DRAWN_BY_FAMILY.get(family, sw.DRAWN_N):
                break
        drawn[family] = keep
        print(family, "drawn:", len(keep), "passed over:", passed)
    return dict(note="written by tests/golden/make_path_sweep.py; see its docstring", seed=sw.SEED, n_paths=sw.N_PATHS,
                cap=sw.CAP, drawn=drawn, cases=cases)


def main():
    doc = build(oracle_ffi.load())
    one = lambda r: json.dumps(r, separators=(",", ":"))  # noqa: E731
    with open(sw.GOLDEN, "w") as f:   # one record per line: a changed digest shows in a diff
        head = {k: v for k, v in doc.items() if k not in ("drawn", "cases")}
        f.write(one(head)[:-1] + ',\n"drawn":{\n')
        f.write(",\n".join(f'"{fam}":[\n' + ",\n".join(one(r) for r in recs) + "\n]" for fam, recs in doc["drawn"].items()))
        f.write('\n},\n"cases":[\n' + ",\n".join(one(r) for r in doc["cases"]) + "\n]}\n")
    print(sw.GOLDEN, os.path.getsize(sw.GOLDEN), "bytes")
    for family in sw.FAMILIES:
        worst = max((max(c["unusable"] for c in r["counts"].values()), r["id"]) for r in doc["cases"] if r["id"].startswith(family + ":"))
        print(f"{family}: largest share left out {worst[0]}/{sw.N_PATHS} ({worst[1]})")


if __name__ == "__main__":
    main()
