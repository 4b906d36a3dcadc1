#!/usr/bin/env python3
"""Kernel time of the Crank–Nicolson grids (hh_fd_solve) by HIP events (hh_ctx_enable_timing), W warm-up calls then K
timed ones per case -> profiles/fd_timing.txt, with hh_crr_solve on the same surface in the same sitting beside them:
  1. one American put and the 32 x 32 American put surface of tools/crr_timing.py, (M, N) = (512, 256) and (1024, 512)
  2. hh_crr_solve, N = 1000 and N = 2000, one put and the same surface
  3. the error of each of the four against the numpy tree oracle averaged over 20000 and 20001 steps, on the six cases
     of tests/fd_cases.py (American puts): cost at equal accuracy
Time per solve step (N + R of them: a Rannacher step is two), the surface's cost against one option's, and the
fraction of an instruction floor: 13 fp64 operations per node-step of a serial solve with the factorisation held
(right-hand side 7, elimination 2, substitution with exercise 4), one VALU lane-instruction each, over 64 lanes, one
wave-instruction per 4 cycles per SIMD on 1024 SIMDs at the sustained clock (profiles/sustained_clock.json).
With --pmc-csv (the counter collection of a run of its own:
    rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -- python3 tools/fd_timing.py --cases-only)
the issued SQ_INSTS_VALU per option-step of each case is set against that count as well.
usage: python tools/fd_timing.py [--warmup W] [--steps K] [--pmc-csv FILE] [--cases-only] [--no-accuracy]"""
import argparse
import collections
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd.pde import fd_device, fd_inputs  # noqa: E402
from hedgehog_jl_amd.trees import crr_device_prices, crr_inputs  # noqa: E402
from oracle import analytic  # noqa: E402
from tests import fd_cases as fc  # noqa: E402
from tools.crr_timing import M as MARKET, REF, surface  # noqa: E402

OPS_PER_NODE_STEP = 13
GRIDS = [(512, 256), (1024, 512)]
TREES = [1000, 2000]
RANNACHER = 2


def one():
    return [hh.VanillaOption(100.0, hh.Date(2021, 1, 1), hh.American(), hh.Put(), hh.Spot())]


def fd_cases_():
    return [(f"{name}, (M, N) = ({M}, {N})", payoffs, M, N) for M, N in GRIDS
            for name, payoffs in (("one American put", one()), ("32 x 32 American put surface", surface()))]


def read_timings(ctx, call, W, K):
    for _ in range(W):
        call()
    ctx.check(ctx.lib.hh_ctx_enable_timing(ctx.handle, 1))
    t0 = time.perf_counter()
    for _ in range(K):
        call()
    wall = (time.perf_counter() - t0) / K * 1e3
    ms = (C.c_double * 256)()
    n = C.c_int32()
    ctx.check(ctx.lib.hh_ctx_read_timings(ctx.handle, ms, 256, C.byref(n)))
    ctx.check(ctx.lib.hh_ctx_enable_timing(ctx.handle, 0))
    return sorted(ms[:n.value]), wall


def valu_by_case(path):
    """SQ_INSTS_VALU per fd_kernel dispatch, in dispatch order (the --cases-only run makes one per case)"""
    rows = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == "SQ_INSTS_VALU" and "fd_kernel" in r["Kernel_Name"]:
            rows[(int(r.get("Dispatch_Id", len(rows))), r["Kernel_Name"])] = float(r["Counter_Value"])
    return [v for _, v in sorted(rows.items())]


def accuracy(lines):
    """American puts of the six cases: each method's distance from the mean of the 20000- and 20001-step trees"""
    lines.append("# |price − oracle|, oracle = mean of oracle/analytic.crr_price at 20000 and 20001 steps (American put), "
                 "per case (S0, K, r, sigma, T)")
    expiry = lambda T: hh.to_ticks(REF) + T * hh.dates.MILLISECONDS_IN_YEAR_365  # noqa: E731
    worst = collections.defaultdict(float)
    for S0, K, r, sigma, T in fc.CASES:
        want = 0.5 * (analytic.crr_price(S0, K, r, sigma, T, 20000, cp=-1.0) + analytic.crr_price(S0, K, r, sigma, T, 20001, cp=-1.0))
        m = hh.BlackScholesInputs(REF, r, S0, sigma)
        prob = hh.PricingProblem(hh.VanillaOption(K, expiry(T), hh.American(), hh.Put(), hh.Spot()), m)
        errs = []
        for Mg, N in GRIDS:
            errs.append((f"CN({Mg}, {N})", abs(hh.solve(prob, hh.CrankNicolsonMethod(Mg, N)).price - want)))
        for N in TREES:
            errs.append((f"CRR({N})", abs(hh.solve(prob, hh.CoxRossRubinsteinMethod(N)).price - want)))
        for k, e in errs:
            worst[k] = max(worst[k], e)
        lines.append(f"{(S0, K, r, sigma, T)}: oracle {want:.8f}; " + ", ".join(f"{k} {e:.2e}" for k, e in errs))
    lines.append("largest over the cases: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--pmc-csv", default=None)
    ap.add_argument("--cases-only", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    a = ap.parse_args()
    ctx = hh.get_context(0)
    if a.cases_only:  # one call per case, nothing else: the dispatches of a counter pass
        for _, payoffs, Mg, N in fd_cases_():
            fd_device(fd_inputs(payoffs, MARKET, hh.CrankNicolsonMethod(Mg, N)), Mg, N, RANNACHER)
        return
    clk = json.load(open(os.path.join(ROOT, "profiles", "sustained_clock.json")))
    mhz = float(np.median([v["clock_mhz"] for k, v in clk.items() if isinstance(v, dict) and "clock_mhz" in v]))
    valu = valu_by_case(a.pmc_csv) if a.pmc_csv else None
    lines = [f"# tools/fd_timing.py --warmup {a.warmup} --steps {a.steps}: hh_fd_solve and hh_crr_solve kernel time by HIP "
             f"events (median / min of K calls), R = {RANNACHER}; floor = {OPS_PER_NODE_STEP} fp64 lane-ops per node-step / 64 "
             f"lanes x 4 cycles / (1024 SIMDs x {mhz:.0f} MHz sustained clock)"]
    single = {}
    for k, (name, payoffs, Mg, N) in enumerate(fd_cases_()):
        inp = fd_inputs(payoffs, MARKET, hh.CrankNicolsonMethod(Mg, N))
        ms, wall = read_timings(ctx, lambda: fd_device(inp, Mg, N, RANNACHER), a.warmup, a.steps)
        med = float(np.median(ms))
        steps = N + RANNACHER
        node_steps = len(payoffs) * (Mg - 1) * steps
        floor_insts = node_steps * OPS_PER_NODE_STEP / 64.0
        floor_ms = floor_insts * 4 / (1024 * mhz * 1e6) * 1e3
        ln = (f"{name}: kernel {med:.4f} ms (min {ms[0]:.4f}), call {wall:.3f} ms wall; {med / steps * 1e3:.3f} us per step "
              f"({med / steps * 1e-3 * mhz * 1e6:.0f} cycles); {node_steps:.3e} node-steps, {node_steps / med * 1e3:.3e} /s; "
              f"floor {floor_ms:.5f} ms -> {floor_ms / med:.4f} of the chip's floor")
        if len(payoffs) == 1:
            single[(Mg, N)] = med
            one_simd = floor_insts * 4 / (mhz * 1e6) * 1e3
            ln += f"; one SIMD's floor {one_simd:.4f} ms -> {one_simd / med:.3f} of it"
        else:
            ln += f"; {med / single[(Mg, N)]:.2f} x the single option's time for {len(payoffs)} options"
        if valu is not None and k < len(valu):
            per = valu[k] / (len(payoffs) * steps)
            need = OPS_PER_NODE_STEP * (Mg - 1) / 64.0
            ln += f"; SQ_INSTS_VALU {valu[k]:.4e} = {per:.1f} per option-step = {per / need:.2f} x the scheme's {need:.1f}"
        lines.append(ln)
    for N in TREES:
        for name, payoffs in (("one American put", one()), ("32 x 32 American put surface", surface())):
            inp = crr_inputs(payoffs, MARKET, N)
            ms, wall = read_timings(ctx, lambda: crr_device_prices(inp, N), a.warmup, a.steps)
            lines.append(f"hh_crr_solve, {name}, N = {N}: kernel {float(np.median(ms)):.4f} ms (min {ms[0]:.4f}), "
                         f"call {wall:.3f} ms wall")
    if not a.no_accuracy:
        accuracy(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "fd_timing.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
