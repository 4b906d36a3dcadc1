#!/usr/bin/env python3
"""The Bates statistics kernel beside its two parents, in the same process and sitting:

  * bates_stats_kernel (the one timing slot of hh_mc_path_stats_bates) at 10^6 x 252, monitored daily and at expiry only,
    plain and antithetic, with and without the martingale correction;
  * qe_stats_kernel (hh_mc_path_stats_qe) on the same model, seeds and shapes;
  * jump_stats_kernel (the first of the two slots of hh_mc_solve_path_jump, one vanilla payoff) on the same seeds, shapes
    and jumps with the lognormal volatility √θ.

Model: κ = 0.3, θ = v₀ = 0.04, σ = 0.9, ρ = −0.5, T = 1, λ = 1, μ_J = −0.1, σ_J = 0.15 — the law test's model scaled to one
year: far from the Feller condition, so the trajectories of a wave sit in both branches of the step, and λ·dt = 1/252, so
nearly every lane leaves the count search at n = 0.  Times are the library's own events (hh_ctx_enable_timing).  Median
of `--reps` calls after `--warmup` calls of the same shape, the whole table twice (two runs in one sitting: their
difference is the spread); the process first runs solves for about a second so that the clocks have ramped before
anything is timed.  The statistics stay in device memory.  One JSON line per row, and a table at the end.  GPU box only.
`--only KERNEL --calls K` runs K calls of one kernel (bates | qe | jump; daily, plain, no correction) and nothing else:
the body of a counter run.

usage: python tools/bates_timing.py [--n 1000000] [--steps 252] [--reps 10] [--warmup 3] [--out FILE]"""
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
ap.add_argument("--only", choices=("bates", "qe", "jump"))
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bates_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS * 2 * n, dtype=torch.float64, device="cuda")
MODEL = dict(S0=100.0, V0=0.04, kappa=0.3, theta=0.04, sigma=0.9, rho=-0.5, r=0.0, T=1.0, strike=100.0, cp=1.0)
m = _ffi.make_model(**MODEL)
m_ln = _ffi.make_model(**dict(MODEL, V0=0.0, kappa=0.0, theta=0.0, rho=0.0, sigma=MODEL["theta"] ** 0.5))
jump = _ffi.make_jump(1.0, -0.1, 0.15)
vanilla = (_ffi.hh_path_payoff * 1)()
vanilla[0].kind, vanilla[0].strike, vanilla[0].cp = _ffi.HH_PAYOFF_VANILLA, 100.0, 1.0
one_result = (_ffi.hh_result * 1)()
lines = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    lines.append(rec)


def slot_of(call, n_slots=1):
    ctx.enable_timing(True)
    call()
    slots = ctx.read_timings()
    ctx.enable_timing(False)
    assert len(slots) == n_slots, slots
    return slots[0]


def median_of(call, n_slots=1):
    return float(np.median([slot_of(call, n_slots) for _ in range(args.warmup + args.reps)][args.warmup:]))


def config(dynamics, strategy, anti):
    c = _ffi.make_config(dynamics, strategy, n, steps, antithetic=anti, em_split=1)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


def qe(c, q, every):
    ctx.check(lib.hh_mc_path_stats_qe(h, C.byref(m), C.byref(q), C.byref(c), every, 0, stats.data_ptr(), 1, None, None))


def bates(c, q, every):
    ctx.check(lib.hh_mc_path_stats_bates(h, C.byref(m), C.byref(q), C.byref(jump), C.byref(c), every, 0, stats.data_ptr(), 1,
                                         None, None))


def merton(c, every):  # two slots: jump_stats_kernel, then the payoff and its reduction
    ctx.check(lib.hh_mc_solve_path_jump(h, C.byref(m_ln), C.byref(jump), C.byref(c), every, 0, vanilla, 1, one_result, None, None))


HES, GBM, QE, EULER = _ffi.HH_HESTON, _ffi.HH_LOGNORMAL, _ffi.HH_QE, _ffi.HH_EULER_MARUYAMA

if args.only:
    cq, cj, q0 = config(HES, QE, 0), config(GBM, EULER, 0), _ffi.make_qe(0.0, 0)
    for _ in range(args.calls):
        {"bates": lambda: bates(cq, q0, 1), "qe": lambda: qe(cq, q0, 1), "jump": lambda: merton(cj, 1)}[args.only]()
    print("ran", args.calls, "calls of", args.only)
    sys.exit(0)

ramp = config(HES, QE, 0)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    qe(ramp, _ffi.make_qe(0.0, 0), steps)

for run in (1, 2):
    for every in (1, steps):
        for anti in (0, 1):
            cq, cj = config(HES, QE, anti), config(GBM, EULER, anti)
            q0, q1 = _ffi.make_qe(0.0, 0), _ffi.make_qe(0.0, 1)
            qe_ms, qe_mart_ms = median_of(lambda: qe(cq, q0, every)), median_of(lambda: qe(cq, q1, every))
            b_ms, b_mart_ms = median_of(lambda: bates(cq, q0, every)), median_of(lambda: bates(cq, q1, every))
            j_ms = median_of(lambda: merton(cj, every), 2)
            emit(dict(run=run, n=n, steps=steps, monitor_every=every, antithetic=anti, qe_stats_ms=round(qe_ms, 4),
                      qe_martingale_stats_ms=round(qe_mart_ms, 4), jump_stats_ms=round(j_ms, 4), bates_stats_ms=round(b_ms, 4),
                      bates_martingale_stats_ms=round(b_mart_ms, 4), ratio=round(b_ms / qe_ms, 3),
                      ratio_martingale=round(b_mart_ms / qe_mart_ms, 3), parents_ratio=round((qe_ms + j_ms) / qe_ms, 3),
                      bates_path_steps_per_s=round(n * steps / (b_ms * 1e-3), 0)))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"Bates statistics kernel beside the quadratic-exponential and the Merton path kernels (tools/bates_timing.py); "
            f"library {os.path.basename(_ffi.LIB_PATH)}\n"
            f"median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's events; two runs in one sitting\n"
            f"kappa 0.3, theta = V0 = 0.04, sigma 0.9, rho -0.5, T 1, lambda 1, mu_J -0.1, sigma_J 0.15; "
            f"ratio = Bates / QE, parents = (QE + jump) / QE\n\n")
    f.write(f"{'run':>3} {'shape':>15} {'every':>5} {'anti':>4} | {'QE':>9} {'QE+mart':>9} {'jump':>9} {'Bates':>9} {'Bates+m':>9} "
            f"{'ratio':>6} {'ratio+m':>7} {'parents':>7}\n")
    for r in lines:
        f.write(f"{r['run']:>3} {str(r['n']) + ' x ' + str(r['steps']):>15} {r['monitor_every']:>5} {r['antithetic']:>4} | "
                f"{r['qe_stats_ms']:>9.4f} {r['qe_martingale_stats_ms']:>9.4f} {r['jump_stats_ms']:>9.4f} {r['bates_stats_ms']:>9.4f} "
                f"{r['bates_martingale_stats_ms']:>9.4f} {r['ratio']:>6.3f} {r['ratio_martingale']:>7.3f} {r['parents_ratio']:>7.3f}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
