"""Writes tests/golden/fd_exact.json: for every run of tests/fd_cases.run_list() the 50-digit price, delta and gamma of
the serial restatement (tests/fd_cases.restate) and the distance e64 of its fp64 run from them.  The large grids take
minutes at 50 digits, so the device test reads this file; tests/test_fd_host.py regenerates a sample of it.

usage: python tests/golden/make_fd_exact.py [processes]"""
import json
import os
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402

from tests import fd_cases as fc  # noqa: E402

DIGITS = 40  # written; e64 is at least 1e-20 of every value, so this loses nothing a bar can see


def record(run):
    exact, e64 = fc.reference(run)
    ci, cp, style, M, N, R, n_std = run
    with mp.workdps(fc.DPS):
        ref = [mp.nstr(x, DIGITS) for x in exact]
    return dict(case=ci, cp=cp, style=style, M=M, N=N, R=R, n_std=n_std, ref=ref, e64=[float(e).hex() for e in e64])


def build(processes=1, runs=None):
    runs = fc.run_list() if runs is None else runs
    if processes > 1:
        with Pool(processes) as pool:
            recs = pool.map(record, sorted(runs, key=lambda r: -r[3] * r[4]), chunksize=1)
        by = {(r["case"], r["cp"], r["style"], r["M"], r["N"], r["R"], r["n_std"]): r for r in recs}
        recs = [by[tuple(r)] for r in runs]
    else:
        recs = [record(r) for r in runs]
    return dict(dps=fc.DPS, digits=DIGITS, cases=[list(c) for c in fc.CASES], runs=recs)


if __name__ == "__main__":
    doc = build(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    with open(fc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(len(doc["runs"]), "runs ->", fc.GOLDEN)
