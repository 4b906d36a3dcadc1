#!/usr/bin/env python3
"""The quadratic-exponential Heston statistics kernel beside the Euler–Maruyama one, in the same process and sitting:

  * qe_stats_kernel (the one timing slot of hh_mc_path_stats_qe) at 10^6 x 252, monitored daily and at expiry only, plain
    and antithetic, with and without the martingale correction;
  * the Heston path_stats_kernel (the one slot of hh_mc_path_stats, em_split = 1) on the same model, seeds and shapes.

Model: κ = 0.3, θ = v₀ = 0.04, σ = 0.9, ρ = −0.5, T = 5 — far from the Feller condition, so the trajectories of a wave
sit in both branches of the step.  Times are the library's own events (hh_ctx_enable_timing).  Median of `--reps` calls
after `--warmup` calls of the same shape, the whole table twice (two runs in one sitting: their difference is the
spread); the process first runs solves for about a second so that the clocks have ramped before anything is timed.  The
statistics stay in device memory.  One JSON line per row, and a table at the end.  GPU box only.

usage: python tools/qe_timing.py [--n 1000000] [--steps 252] [--reps 10] [--warmup 3] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qe_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS * 2 * n, dtype=torch.float64, device="cuda")
m = _ffi.make_model(S0=100.0, V0=0.04, kappa=0.3, theta=0.04, sigma=0.9, rho=-0.5, r=0.0, T=5.0, strike=100.0, cp=1.0)
lines = []


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


def config(strategy, anti):
    c = _ffi.make_config(_ffi.HH_HESTON, strategy, n, steps, antithetic=anti, em_split=1)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


def euler(c, every):
    ctx.check(lib.hh_mc_path_stats(h, C.byref(m), C.byref(c), every, 0, stats.data_ptr(), 1, None))


def qe(c, q, every):
    ctx.check(lib.hh_mc_path_stats_qe(h, C.byref(m), C.byref(q), C.byref(c), every, 0, stats.data_ptr(), 1, None, None))


ramp = config(_ffi.HH_EULER_MARUYAMA, 0)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    euler(ramp, steps)

for run in (1, 2):
    for every in (1, steps):
        for anti in (0, 1):
            ce, cq = config(_ffi.HH_EULER_MARUYAMA, anti), config(_ffi.HH_QE, anti)
            euler_ms = median_of(lambda: euler(ce, every))
            plain_ms = median_of(lambda: qe(cq, _ffi.make_qe(0.0, 0), every))
            mart_ms = median_of(lambda: qe(cq, _ffi.make_qe(0.0, 1), every))
            emit(dict(run=run, n=n, steps=steps, monitor_every=every, antithetic=anti, euler_stats_ms=round(euler_ms, 4),
                      qe_stats_ms=round(plain_ms, 4), qe_martingale_stats_ms=round(mart_ms, 4),
                      ratio=round(plain_ms / euler_ms, 3), ratio_martingale=round(mart_ms / euler_ms, 3),
                      qe_path_steps_per_s=round(n * steps / (plain_ms * 1e-3), 0)))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"Quadratic-exponential Heston statistics kernel beside the Euler–Maruyama one (tools/qe_timing.py); library "
            f"{os.path.basename(_ffi.LIB_PATH)}\n"
            f"median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's events; two runs in one sitting\n"
            f"kappa 0.3, theta = V0 = 0.04, sigma 0.9, rho -0.5, T 5\n\n")
    f.write(f"{'run':>3} {'shape':>15} {'every':>5} {'anti':>4} | {'Euler':>9} {'QE':>9} {'QE+mart':>9} {'ratio':>6} {'ratio+m':>7}\n")
    for r in lines:
        f.write(f"{r['run']:>3} {str(r['n']) + ' x ' + str(r['steps']):>15} {r['monitor_every']:>5} {r['antithetic']:>4} | "
                f"{r['euler_stats_ms']:>9.4f} {r['qe_stats_ms']:>9.4f} {r['qe_martingale_stats_ms']:>9.4f} {r['ratio']:>6.3f} "
                f"{r['ratio_martingale']:>7.3f}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
