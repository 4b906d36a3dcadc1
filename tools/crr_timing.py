#!/usr/bin/env python3
"""Kernel time of the Cox–Ross–Rubinstein trees (hh_crr_solve) by HIP events (hh_ctx_enable_timing), W warm-up
calls then K timed ones per case -> profiles/crr_timing.txt:
  1. one American put, N = 1000
  2. a 32 x 32 strike/expiry surface of American puts in ONE call, N = 1000 and N = 2000
  3. one tree with N = 32768 (form B)
  4. the numpy oracle (oracle/analytic.crr_price) on a sample of the trees of (2), extrapolated to the surface
Node updates per second, and the fraction of an instruction floor: ~4 fp64 operations per node-step (European) or
~9 (American: continuation plus exercise), one VALU lane-instruction each, over 64 lanes, issued at one
wave-instruction per 4 cycles per SIMD on 1024 SIMDs at the sustained clock (profiles/sustained_clock.json).
With --pmc-csv (the counter collection of a run of its own:
    rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -- python3 tools/crr_timing.py --cases-only)
the issued SQ_INSTS_VALU of each case is set against that floor as well.
usage: python tools/crr_timing.py [--warmup W] [--steps K] [--pmc-csv FILE] [--cases-only]"""
import argparse
import collections
import csv
import ctypes as C
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd.trees import crr_device_prices, crr_inputs  # noqa: E402
from oracle import analytic  # noqa: E402

REF = hh.Date(2020, 1, 1)
M = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.25)


def surface(n=32):
    strikes = np.linspace(70.0, 130.0, n)
    expiries = [REF + datetime.timedelta(days=int(d)) for d in np.linspace(30, 730, n)]
    return [hh.VanillaOption(float(K), e, hh.American(), hh.Put(), hh.Spot()) for e in expiries for K in strikes]


def cases():
    one = [hh.VanillaOption(100.0, hh.Date(2021, 1, 1), hh.American(), hh.Put(), hh.Spot())]
    return [("one American put, N = 1000", one, 1000), ("32 x 32 American put surface, N = 1000", surface(), 1000),
            ("32 x 32 American put surface, N = 2000", surface(), 2000),
            ("one American put, N = 32768 (form B)", one, 32768)]


def timed(ctx, inp, N, W, K):
    for _ in range(W):
        crr_device_prices(inp, N)
    ctx.check(ctx.lib.hh_ctx_enable_timing(ctx.handle, 1))
    t0 = time.perf_counter()
    for _ in range(K):
        crr_device_prices(inp, N)
    wall = (time.perf_counter() - t0) / K * 1e3
    ms = (C.c_double * 256)()
    n = C.c_int32()
    ctx.check(ctx.lib.hh_ctx_read_timings(ctx.handle, ms, 256, C.byref(n)))
    ctx.check(ctx.lib.hh_ctx_enable_timing(ctx.handle, 0))
    return sorted(ms[:n.value]), wall


def valu_by_case(path):
    """SQ_INSTS_VALU per crr_kernel dispatch, in dispatch order (the --cases-only run makes one per case)"""
    rows = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == "SQ_INSTS_VALU" and "crr_kernel" in r["Kernel_Name"]:
            rows[(int(r.get("Dispatch_Id", len(rows))), r["Kernel_Name"])] = float(r["Counter_Value"])
    return [v for _, v in sorted(rows.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pmc-csv", default=None)
    ap.add_argument("--cases-only", action="store_true")
    a = ap.parse_args()
    ctx = hh.get_context(0)
    if a.cases_only:  # one call per case, nothing else: the dispatches of a counter pass
        for _, payoffs, N in cases():
            crr_device_prices(crr_inputs(payoffs, M, N), N)
        return
    clk = json.load(open(os.path.join(ROOT, "profiles", "sustained_clock.json")))
    mhz = float(np.median([v["clock_mhz"] for k, v in clk.items() if isinstance(v, dict) and "clock_mhz" in v]))
    valu = valu_by_case(a.pmc_csv) if a.pmc_csv else None
    lines = [f"# tools/crr_timing.py --warmup {a.warmup} --steps {a.steps}: hh_crr_solve kernel time by HIP events "
             f"(median / min of K calls); floor = 9 fp64 lane-ops per American node-step / 64 lanes x 4 cycles / "
             f"(1024 SIMDs x {mhz:.0f} MHz sustained clock)"]
    surf_ms = {}
    for k, (name, payoffs, N) in enumerate(cases()):
        inp = crr_inputs(payoffs, M, N)
        ms, wall = timed(ctx, inp, N, a.warmup, a.steps)
        med = float(np.median(ms))
        nodes = len(payoffs) * N * (N + 1) / 2
        floor_insts = nodes * 9 / 64.0
        floor_ms = floor_insts * 4 / (1024 * mhz * 1e6) * 1e3
        ln = (f"{name}: kernel {med:.4f} ms (min {ms[0]:.4f}), call {wall:.3f} ms wall; {nodes:.3e} node updates, "
              f"{nodes / med * 1e3:.3e} /s; floor {floor_ms:.5f} ms -> {floor_ms / med:.3f} of the chip's floor")
        if valu is not None and k < len(valu):
            ln += f"; SQ_INSTS_VALU {valu[k]:.4e} = {valu[k] / floor_insts:.2f} x the floor's {floor_insts:.4e}"
        lines.append(ln)
        if len(payoffs) > 1:
            surf_ms[N] = med
    # 4. the numpy oracle on a sample of the surface's trees, extrapolated
    surf = surface()
    sample = surf[::64]
    for N in (1000, 2000):
        t0 = time.perf_counter()
        for p in sample:
            T = hh.yearfrac(REF, p.expiry)
            analytic.crr_price(100.0, p.strike, 0.05, 0.25, T, N, cp=-1.0)
        per = (time.perf_counter() - t0) / len(sample) * 1e3
        lines.append(f"numpy oracle, N = {N}: {per:.2f} ms per tree on the host ({len(sample)} sampled) -> "
                     f"{per * len(surf) / 1e3:.2f} s for the 1024-tree surface; the device surface is "
                     f"{per * len(surf) / surf_ms[N]:.0f}x faster")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "crr_timing.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
