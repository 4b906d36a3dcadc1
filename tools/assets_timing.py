#!/usr/bin/env python3
"""The multi-asset statistics kernel beside the lognormal one, in the same process and sitting:

  * assets_stats_kernel (slot 0 of hh_mc_solve_path_assets) at 10^6 x 252, monitored daily, for d = 1, 2, 4, 8 assets
    (C_ij = 0.5^|i-j|) and each index kind, with and without antithetic;
  * path_stats_kernel on lognormal dynamics (slot 0 of hh_mc_solve_path) at the same shape.

The table gives each time's ratio to the lognormal kernel beside what the algorithm predicts from the lognormal kernel's
own instruction mix: per path-step the lognormal kernel draws half a Philox block and half a Box–Muller pair and takes
one fma-step and one exp; the asset kernel draws ceil(d/2) of each, takes d(d+1)/2 fma (twice with the mirror) and d exp
and one log (weighted sum) or one exp (the other kinds) per date.  `--pmc-shape` runs only the d = 1 and d = 4 weighted
sums and the lognormal kernel once each, for a counter collection (rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES) of its own.

Times are the library's own events (hh_ctx_enable_timing).  Median of `--reps` calls after `--warmup` calls of the same
shape, the whole table twice (two runs in one sitting: their difference is the spread); the process first runs solves
for about a second so that the clocks have ramped before anything is timed.  One JSON line per row, and a table at the
end.  GPU box only.

usage: python tools/assets_timing.py [--n 1000000] [--steps 252] [--reps 10] [--warmup 3] [--out FILE] [--pmc-shape]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hedgehog_jl_amd import _ffi

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=252)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assets_timing.txt"))
ap.add_argument("--pmc-shape", action="store_true")
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
m = _ffi.make_model(S0=100.0, sigma=0.2, r=0.03, T=1.0, strike=105.0, cp=1.0)
KINDS = {0: "weighted sum", 1: "geometric", 2: "best of", 3: "worst of"}
lines = []
pay, out = (_ffi.hh_path_payoff * 1)(), (_ffi.hh_result * 1)()
pay[0].kind, pay[0].strike, pay[0].cp = _ffi.HH_PAYOFF_VANILLA, 105.0, 1.0


def emit(rec):
    print(json.dumps(rec), flush=True)
    lines.append(rec)


def slots_of(call, want):
    ctx.enable_timing(True)
    call()
    slots = ctx.read_timings()
    ctx.enable_timing(False)
    assert len(slots) == want, slots
    return slots


def median_of(call):
    rows = [call() for _ in range(args.warmup + args.reps)][args.warmup:]
    return [float(np.median([r[i] for r in rows])) for i in range(len(rows[0]))]


def config(anti):
    c = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, n, steps, antithetic=anti)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


def assets(d, kind):
    return _ffi.make_assets([100.0 + i for i in range(d)], [0.2 + 0.02 * i for i in range(d)], [1.0 / d] * d,
                            [[0.5 ** abs(i - j) for j in range(d)] for i in range(d)], kind)


def lognormal(c):
    return lambda: ctx.check(lib.hh_mc_solve_path(h, C.byref(m), C.byref(c), 1, 0, pay, 1, out, None, None))


def multi(a, c):
    return lambda: ctx.check(lib.hh_mc_solve_path_assets(h, C.byref(m), C.byref(a), C.byref(c), 1, 0, pay, 1, out, None, None))


def predicted(d, kind, anti):
    """The asset kernel's VALU instructions per path-step over the lognormal kernel's, daily dates.  The units are read
    off the disassembly of assets_stats_kernel<8, 1, false>'s loop (561 VALU instructions: four Philox blocks with their
    Box–Muller pairs, 36 fma and 8 additions of the step, 8 fma of the index, one exp, the statistics, 26 lane reads):
    BLOCK = 116 for one block and pair, EXP = 40 for one exp (a log taken as one), REST = 8 for the statistics and the
    date.  They give the lognormal kernel 58 + 2 + 40 + 8 = 108 against the 107 it measures."""
    BLOCK, EXP, REST = 116.0, 40.0, 8.0
    members = 2 if anti else 1
    per_member = d * (d + 1) / 2 + d + (0 if kind == 0 else d - 1) + EXP * ((d + 1) if kind == 0 else 1) + REST
    base = BLOCK / 2 + members * (2 + EXP + REST)
    return (BLOCK * ((d + 1) // 2) + members * per_member) / base


if args.pmc_shape:
    c = config(0)
    lognormal(c)()
    for d in (1, 4):
        multi(assets(d, 0), c)()
    print("pmc shape: path_stats_kernel, assets_stats_kernel<1, 0, false>, assets_stats_kernel<4, 0, false> once each at "
          f"{n} x {steps}")
    sys.exit(0)

# clock ramp: lognormal path solves for about a second
ramp = config(0)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    lognormal(ramp)()

for run in (1, 2):
    for anti in (0, 1):
        c = config(anti)
        logn = median_of(lambda: slots_of(lognormal(c), 2))
        emit(dict(what="lognormal", run=run, n=n, steps=steps, antithetic=anti, stats_ms=round(logn[0], 4),
                  payoff_kernels_ms=round(logn[1], 4)))
        for d in (1, 2, 4, 8):
            for kind in KINDS:
                a = assets(d, kind)
                t = median_of(lambda: slots_of(multi(a, c), 2))
                emit(dict(what="assets", run=run, n=n, steps=steps, antithetic=anti, d=d, kind=KINDS[kind],
                          stats_ms=round(t[0], 4), ratio=round(t[0] / logn[0], 3), predicted=round(predicted(d, kind, anti), 2),
                          asset_steps_per_s=round(n * steps * d / (t[0] * 1e-3), 0)))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"The multi-asset statistics kernel beside the lognormal one (tools/assets_timing.py); library {os.path.basename(_ffi.LIB_PATH)}\n"
            f"{n} x {steps}, monitored daily; median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's "
            "events; two runs in one sitting\nratio: to path_stats_kernel on lognormal dynamics, same run and member count; "
            "predicted: from the lognormal kernel's instruction mix (see the tool)\n\n")
    f.write(f"{'run':>3} {'anti':>4} {'d':>2} {'index':>13} | {'ms':>9} {'ratio':>7} {'predicted':>9}\n")
    for r in lines:
        if r["what"] == "lognormal":
            f.write(f"{r['run']:>3} {r['antithetic']:>4} {'-':>2} {'(lognormal)':>13} | {r['stats_ms']:>9.4f} {1.0:>7.3f} {'':>9}\n")
        else:
            f.write(f"{r['run']:>3} {r['antithetic']:>4} {r['d']:>2} {r['kind']:>13} | {r['stats_ms']:>9.4f} {r['ratio']:>7.3f} "
                    f"{r['predicted']:>9.2f}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
