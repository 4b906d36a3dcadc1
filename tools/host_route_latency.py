#!/usr/bin/env python3
"""Microseconds of Python in front of a Monte Carlo call, per hh.solve, through the recording context of
tests/route_cases.py (no GPU: the C entry point is a function that logs its arguments).

    python tools/host_route_latency.py [--package-root DIR] [--case NAME] [--calls 2000] [--warmup 200] [--repeats 5]

--package-root: the directory whose hedgehog_jl_amd is measured (default: this checkout), to put two commits side by side;
--case with --repeats 1 lets a driver take the two commits' repeats in turn, which a machine whose speed drifts needs."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--case", default="")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.package_root), ROOT]
    from tests import route_cases as rc
    hh = rc.hh
    assert os.path.dirname(os.path.abspath(hh.__file__)) == os.path.abspath(a.package_root), hh.__file__
    R, cases = rc.ROUTES, rc.cases()
    rows = {"plain European": dict(R["plain"]["spec"], skw=dict(ensemble=False)),
            "Euler Asian": dict(R["euler"]["spec"], skw=dict(ensemble=False)),
            "Bates vanilla": dict(R["bates"]["spec"], payoffs=[rc.vanilla()], skw=dict(ensemble=False)),
            "local-vol barrier": dict(R["localvol"]["spec"], skw=dict(ensemble=False)),
            "multi-asset option": dict(R["multiasset"]["spec"], skw=dict(ensemble=False)),
            "mixed basket": cases["basket/euler_mixed/ensemble=False"]}
    print(f"package {os.path.dirname(hh.__file__)}: us per hh.solve, {a.calls} calls after {a.warmup}, {a.repeats} repeats")
    print(f"{'case':<20}{'median':>9}{'min':>9}{'max':>9}")
    for name, spec in rows.items():
        if a.case not in name:
            continue
        spec = dict(spec, method=rc.mc(spec["dyn"], spec["strat"], spec["steps"], anti=spec.get("anti", False)))
        with rc.recording(log=False):
            us = []
            for _ in range(a.repeats):
                for _ in range(a.warmup):
                    rc.execute(spec)
                t = time.perf_counter()
                for _ in range(a.calls):
                    rc.execute(spec)
                us.append((time.perf_counter() - t) / a.calls * 1e6)
        print(f"{name:<20}{statistics.median(us):9.1f}{min(us):9.1f}{max(us):9.1f}")


if __name__ == "__main__":
    main()
