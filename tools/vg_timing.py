#!/usr/bin/env python3
"""Variance Gamma beside the Merton and lognormal kernels, in the same process and sitting:

  * the terminal law (hh_mc_solve_vg, θ = −0.3, ν = 0.5: shape 2) at 10^6 and 10^8 trajectories beside merton_exact_kernel
    (hh_mc_solve_jump, λ = 0.8) — one timing slot each: the simulation kernel with its record reduction;
  * vg_stats_kernel (slot 0 of hh_mc_solve_path_vg) at 10^6 x 12 and x 252, monitored at every step, ν = 0.2 and 0.5, with
    and without antithetic, beside jump_stats_kernel (λ = 1) and the lognormal path_stats_kernel on the same seeds.

The mean number of attempt rounds a WAVE makes per variate is derived, not counted: a lane accepts an attempt with
probability p (estimated here from the host's own sampler on 2^16 draws per shape: csrc/hh_vg.h is the same code), the
wave goes on until its slowest lane has accepted, so rounds = Σ_k (1 − (1 − (1 − p)^k)^64).

Times are the library's own events (hh_ctx_enable_timing).  Median of `--reps` calls after `--warmup` calls of the same
shape, the whole table twice (two runs in one sitting: their difference is the spread); the process first runs solves for
about a second so that the clocks have ramped before anything is timed.  One JSON line per row, and a table at the end.
GPU box only.

usage: python tools/vg_timing.py [--n 1000000] [--big 100000000] [--reps 10] [--warmup 3] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vg_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n = args.n
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


def wave_rounds(shape):
    """expected attempts of the slowest of 64 lanes; the acceptance p of Marsaglia–Tsang at this shape by simulation"""
    rng = np.random.default_rng(1)
    a1 = shape + 1.0 if shape < 1.0 else shape
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    z, U = rng.standard_normal(2 ** 20), rng.random(2 ** 20)
    v = (1.0 + c * z) ** 3
    ok = v > 0.0
    acc = np.zeros_like(ok)
    acc[ok] = np.log(U[ok]) < 0.5 * z[ok] ** 2 + d - d * v[ok] + d * np.log(v[ok])
    p = float(acc.mean())
    return p, float(sum(1.0 - (1.0 - (1.0 - p) ** k) ** 64 for k in range(64)))


# clock ramp: exact-law solves for about a second
ramp = exact_config(n)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(ramp), C.byref(res), None))

for run in (1, 2):
    jump, vg = _ffi.make_jump(0.8, -0.1, 0.15), _ffi.make_vg(-0.3, 0.5)
    for k in (n, args.big):
        c = exact_config(k)
        (jump_ms,) = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_jump(h, C.byref(m), C.byref(jump), C.byref(c), C.byref(res), None)), 1))
        (vg_ms,) = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_vg(h, C.byref(m), C.byref(vg), C.byref(c), C.byref(res), None)), 1))
        p, rounds = wave_rounds(m.T / vg.nu)
        emit(dict(what="terminal", run=run, n=k, merton_exact_ms=round(jump_ms, 4), vg_exact_ms=round(vg_ms, 4),
                  ratio=round(vg_ms / jump_ms, 3), vg_trajectories_per_s=round(k / (vg_ms * 1e-3), 0), acceptance=round(p, 4),
                  wave_rounds=round(rounds, 3)))
    jump = _ffi.make_jump(1.0, -0.1, 0.15)
    pay, out = (_ffi.hh_path_payoff * 1)(), (_ffi.hh_result * 1)()
    pay[0].kind, pay[0].strike, pay[0].cp = _ffi.HH_PAYOFF_VANILLA, 105.0, 1.0
    for steps in (12, 252):
        for anti in (0, 1):
            ce = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, n, steps, antithetic=anti)
            cx = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW, n, steps, antithetic=anti)
            for c in (ce, cx):
                c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
            logn = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_path(h, C.byref(m), C.byref(ce), 1, 0, pay, 1, out, None, None)), 2))
            jmp = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_path_jump(h, C.byref(m), C.byref(jump), C.byref(ce), 1, 0, pay, 1, out, None, None)), 2))
            for nu in (0.2, 0.5):
                vg = _ffi.make_vg(-0.3, nu)
                v = median_of(lambda: slots_of(lambda: ctx.check(lib.hh_mc_solve_path_vg(h, C.byref(m), C.byref(vg), C.byref(cx), 1, 0, pay, 1, out, None, None)), 2))
                p, rounds = wave_rounds(m.T / steps / nu)
                emit(dict(what="path", run=run, n=n, steps=steps, antithetic=anti, nu=nu, shape=round(m.T / steps / nu, 5),
                          lognormal_stats_ms=round(logn[0], 4), jump_stats_ms=round(jmp[0], 4), vg_stats_ms=round(v[0], 4),
                          vs_lognormal=round(v[0] / logn[0], 3), vs_jump=round(v[0] / jmp[0], 3), acceptance=round(p, 4),
                          wave_rounds=round(rounds, 3), vg_path_steps_per_s=round(n * steps / (v[0] * 1e-3), 0)))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"Variance Gamma beside the Merton and lognormal kernels (tools/vg_timing.py); library {os.path.basename(_ffi.LIB_PATH)}\n"
            f"median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's events; two runs in one sitting\n"
            "wave rounds per variate: derived from the acceptance of one attempt (the tool's docstring), not counted\n\n")
    f.write(f"{'run':>3} {'terminal law, n':>16} | {'Merton':>10} {'VG':>10} {'ratio':>6} {'rounds':>7}\n")
    for r in lines:
        if r["what"] == "terminal":
            f.write(f"{r['run']:>3} {r['n']:>16} | {r['merton_exact_ms']:>10.4f} {r['vg_exact_ms']:>10.4f} {r['ratio']:>6.3f} {r['wave_rounds']:>7.3f}\n")
    f.write(f"\n{'run':>3} {'statistics kernel':>17} {'anti':>4} {'nu':>4} | {'lognormal':>10} {'jump':>10} {'VG':>10} {'/logn':>6} {'/jump':>6} {'rounds':>7}\n")
    for r in lines:
        if r["what"] == "path":
            f.write(f"{r['run']:>3} {str(r['n']) + ' x ' + str(r['steps']):>17} {r['antithetic']:>4} {r['nu']:>4} | {r['lognormal_stats_ms']:>10.4f} "
                    f"{r['jump_stats_ms']:>10.4f} {r['vg_stats_ms']:>10.4f} {r['vs_lognormal']:>6.2f} {r['vs_jump']:>6.2f} {r['wave_rounds']:>7.3f}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
