#!/usr/bin/env python3
"""Merton jump diffusion beside its lognormal counterparts, in the same process and sitting:

  * the terminal law (hh_mc_solve_jump, λ = 0.8) at 10^6 and 10^8 trajectories beside the exact lognormal law
    (hh_mc_solve, HH_EXACT_LAW) — one timing slot each: the simulation kernel with its record reduction;
  * the jump statistics kernel (slot 0 of hh_mc_solve_path_jump, λ = 1, so λ·dt = 1/252) at 10^6 x 252, monitored daily,
    beside the lognormal statistics kernel (slot 0 of hh_mc_solve_path), with and without antithetic.

Times are the library's own events (hh_ctx_enable_timing).  Median of `--reps` calls after `--warmup` calls of the same
shape, the whole table twice (two runs in one sitting: their difference is the spread); the process first runs solves
for about a second so that the clocks have ramped before anything is timed.  One JSON line per row, and a table at the
end.  GPU box only.

usage: python tools/jump_timing.py [--n 1000000] [--big 100000000] [--steps 252] [--reps 10] [--warmup 3] [--out FILE]"""
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
ap.add_argument("--big", type=int, default=100_000_000)
ap.add_argument("--steps", type=int, default=252)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jump_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
m = _ffi.make_model(S0=100.0, sigma=0.2, r=0.03, T=1.0, strike=105.0, cp=1.0)
res = _ffi.hh_result()
lines = []


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


def exact_config(k):
    c = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW, k, 1)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, 1
    return c


# clock ramp: exact-law solves for about a second
ramp = exact_config(n)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(ramp), C.byref(res), None))

for run in (1, 2):
    jump = _ffi.make_jump(0.8, -0.1, 0.15)
    for k in (n, args.big):
        c = exact_config(k)
        (logn_ms,) = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(c), C.byref(res), None)), 1))
        (jump_ms,) = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_jump(h, C.byref(m), C.byref(jump), C.byref(c), C.byref(res), None)), 1))
        emit(dict(what="terminal", run=run, n=k, lognormal_exact_ms=round(logn_ms, 4), merton_exact_ms=round(jump_ms, 4),
                  ratio=round(jump_ms / logn_ms, 3), merton_trajectories_per_s=round(k / (jump_ms * 1e-3), 0)))
    jump = _ffi.make_jump(1.0, -0.1, 0.15)
    pay, out = (_ffi.hh_path_payoff * 1)(), (_ffi.hh_result * 1)()
    pay[0].kind, pay[0].strike, pay[0].cp = _ffi.HH_PAYOFF_VANILLA, 105.0, 1.0
    for anti in (0, 1):
        c = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, n, steps, antithetic=anti)
        c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
        logn = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_path(h, C.byref(m), C.byref(c), 1, 0, pay, 1, out, None, None)), 2))
        jmp = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_path_jump(h, C.byref(m), C.byref(jump), C.byref(c), 1, 0, pay, 1, out, None, None)), 2))
        emit(dict(what="path", run=run, n=n, steps=steps, antithetic=anti, lognormal_stats_ms=round(logn[0], 4),
                  jump_stats_ms=round(jmp[0], 4), ratio=round(jmp[0] / logn[0], 3), payoff_kernels_ms=round(jmp[1], 4),
                  jump_path_steps_per_s=round(n * steps / (jmp[0] * 1e-3), 0)))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"Merton jump diffusion beside the lognormal kernels (tools/jump_timing.py); library {os.path.basename(_ffi.LIB_PATH)}\n"
            f"median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's events; two runs in one sitting\n\n")
    f.write(f"{'run':>3} {'terminal law, n':>16} | {'lognormal':>10} {'Merton':>10} {'ratio':>6}\n")
    for r in lines:
        if r["what"] == "terminal":
            f.write(f"{r['run']:>3} {r['n']:>16} | {r['lognormal_exact_ms']:>10.4f} {r['merton_exact_ms']:>10.4f} {r['ratio']:>6.3f}\n")
    f.write(f"\n{'run':>3} {'statistics kernel':>17} {'anti':>4} | {'lognormal':>10} {'jump':>10} {'ratio':>6}\n")
    for r in lines:
        if r["what"] == "path":
            f.write(f"{r['run']:>3} {str(r['n']) + ' x ' + str(r['steps']):>17} {r['antithetic']:>4} | {r['lognormal_stats_ms']:>10.4f} "
                    f"{r['jump_stats_ms']:>10.4f} {r['ratio']:>6.3f}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
