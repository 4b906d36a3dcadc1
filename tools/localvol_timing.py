#!/usr/bin/env python3
"""The local-volatility statistics kernel beside the lognormal one, in the same process and sitting:

  * localvol_stats_kernel (the one timing slot of hh_mc_path_stats_lv) at 10^6 x 252, monitored daily and at expiry only,
    plain, antithetic and in the bridge form, on tables of (n_times, n_x) = (1, 64), (16, 128) and (32, 256) nodes —
    0.5 KiB, 16 KiB and the full 64 KiB of LDS per workgroup;
  * the lognormal path_stats_kernel (the one slot of hh_mc_path_stats_ex, sigma = 0.25) on the same seeds and shapes.

Surface: σ0·(S/S0)^{−1/2}·(1 + 0.1·t) with σ0 = 0.25 on log S0 ± 1.5, times spread over (0, 1]; S0 = 100, r = 0.03, T = 1 —
the lanes of a wave cluster at the money, as they do in use.  Times are the library's own events
(hh_ctx_enable_timing).  Median of `--reps` calls after `--warmup` calls of the same shape, the whole table twice (two
runs in one sitting: their difference is the spread); the process first runs solves for about a second so that the
clocks have ramped before anything is timed.  The statistics stay in device memory.  One JSON line per row, and a table
at the end.  `--pmc-shape` runs every kernel once, daily, in a fixed order, for a counter collection of its own
(rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE, nothing traced).  GPU box only.

usage: python tools/localvol_timing.py [--n 1000000] [--steps 252] [--reps 10] [--warmup 3] [--out FILE] [--pmc-shape]"""
import argparse
import ctypes as C
import json
import math
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
ap.add_argument("--pmc-shape", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localvol_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS_BRIDGE * 2 * n, dtype=torch.float64, device="cuda")
m = _ffi.make_model(S0=100.0, V0=0.0, kappa=0.0, theta=0.0, sigma=0.25, rho=0.0, r=0.03, T=1.0, strike=100.0, cp=1.0)
TABLES = ((1, 64), (16, 128), (32, 256))
FORMS = (("plain", 0, _ffi.HH_EXTREMES_MONITORED), ("antithetic", 1, _ffi.HH_EXTREMES_MONITORED),
         ("bridge", 0, _ffi.HH_EXTREMES_BRIDGE))
lines = []


def table(n_t, n_x):
    x0 = math.log(100.0)
    x = x0 - 1.5 + 3.0 / (n_x - 1) * np.arange(n_x)
    times = np.arange(1, n_t + 1) / n_t
    vols = 0.25 * np.exp(-0.5 * (x - x0))[None, :] * (1.0 + 0.1 * times)[:, None]
    return _ffi.make_localvol(times, vols, x[0], 3.0 / (n_x - 1))


surfaces = {t: table(*t) for t in TABLES}


def emit(rec):
    print(json.dumps(rec), flush=True)
    lines.append(rec)


def slot_of(call):
    ctx.enable_timing(True)
    call()
    slots = ctx.read_timings()
    ctx.enable_timing(False)
    assert len(slots) == 1, slots
    return slots[0]


def median_of(call):
    return float(np.median([slot_of(call) for _ in range(args.warmup + args.reps)][args.warmup:]))


def config(anti):
    c = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, n, steps, antithetic=anti)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


def lognormal(c, every, extremes):
    ctx.check(lib.hh_mc_path_stats_ex(h, C.byref(m), C.byref(c), every, 0, extremes, stats.data_ptr(), 1, None))


def localvol(c, lv, every, extremes):
    ctx.check(lib.hh_mc_path_stats_lv(h, C.byref(m), C.byref(lv), C.byref(c), every, 0, extremes, stats.data_ptr(), 1, None))


if args.pmc_shape:  # once each, in this order, for a counter collection of its own (rocprofv3 --pmc …, nothing traced)
    for _, anti, extremes in FORMS:
        c = config(anti)
        lognormal(c, 1, extremes)
        for t in TABLES:
            localvol(c, surfaces[t], 1, extremes)
    print(f"pmc shape: per form (plain, antithetic, bridge) path_stats_kernel, then localvol_stats_kernel on {TABLES}, once "
          f"each at {n} x {steps}, daily")
    sys.exit(0)

ramp = config(0)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    lognormal(ramp, steps, _ffi.HH_EXTREMES_MONITORED)

for run in (1, 2):
    for every in (1, steps):
        for form, anti, extremes in FORMS:
            c = config(anti)
            logn_ms = median_of(lambda: lognormal(c, every, extremes))
            rec = dict(run=run, n=n, steps=steps, monitor_every=every, form=form, lognormal_stats_ms=round(logn_ms, 4))
            for t in TABLES:
                ms = median_of(lambda: localvol(c, surfaces[t], every, extremes))
                rec[f"lv_{t[0]}x{t[1]}_ms"] = round(ms, 4)
                rec[f"ratio_{t[0]}x{t[1]}"] = round(ms / logn_ms, 3)
            emit(rec)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"Local-volatility statistics kernel beside the lognormal one (tools/localvol_timing.py); library "
            f"{os.path.basename(_ffi.LIB_PATH)}\n"
            f"median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's events; two runs in one sitting\n"
            f"sigma0 0.25, S0 100, r 0.03, T 1; tables (n_times, n_x) over log S0 +- 1.5: LDS per workgroup 0.5, 16 and 64 KiB\n\n")
    f.write(f"{'run':>3} {'shape':>15} {'every':>5} {'form':>10} | {'lognormal':>9} " +
            " ".join(f"{'lv ' + str(t[0]) + 'x' + str(t[1]):>9} {'ratio':>6}" for t in TABLES) + "\n")
    for r in lines:
        f.write(f"{r['run']:>3} {str(r['n']) + ' x ' + str(r['steps']):>15} {r['monitor_every']:>5} {r['form']:>10} | "
                f"{r['lognormal_stats_ms']:>9.4f} " +
                " ".join(f"{r[f'lv_{t[0]}x{t[1]}_ms']:>9.4f} {r[f'ratio_{t[0]}x{t[1]}']:>6.3f}" for t in TABLES) + "\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
