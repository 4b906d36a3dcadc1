#!/usr/bin/env python3
"""The date-row form of the log-spot path family beside its statistics form, and the LSM induction behind it, in the same
process and sitting:

  * per source (Euler lognormal and Heston, Merton jumps, QE, Bates, local volatility on a 16 × 128 table, Variance Gamma)
    the statistics kernel — the one timing slot of the source's hh_mc_path_stats* call — at monitor_every = e, and the
    date-row kernel — the one slot of hh_mc_path_grid — at exercise_every = e, for e = steps/12 and e = 1 (12 and `steps`
    dates), plain and antithetic;
  * hh_lsm_solve_path on the same shape, degree 3: its kernel_ms (grid and induction, first event to last) less the grid's.

The expectation tested: grid <= statistics + the time to write 8·n_total·(n_dates + 1) bytes at 6.99 TB/s, the rate
README's headline reaches.  `excess_ms` is what the grid takes beyond that (negative: inside it).

Times are the library's own events (hh_ctx_enable_timing).  Median of `--reps` calls after `--warmup` calls of the same
shape, the whole table twice (two runs in one sitting: their difference is the spread); the process first runs solves for
about a second so that the clocks have ramped before anything is timed.  Statistics and grids stay in device memory.
One JSON line per row, and a table at the end, written to profiles/path_grid_timing_table.txt — the table and rows that
profiles/path_grid_timing.txt quotes in its sections 3 and 4 beside what no tool writes (the disassembly comparison, the
register report).  GPU box only.

usage: python tools/path_grid_timing.py [--n 1000000] [--steps 252] [--reps 5] [--warmup 2] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_grid_timing_table.txt"))
args = ap.parse_args()

HBM_RATE = 6.99e12  # bytes/s: README's headline
ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS * 2 * n, dtype=torch.float64, device="cuda")
GBM, HES = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON
EM, QE, LAW = _ffi.HH_EULER_MARUYAMA, _ffi.HH_QE, _ffi.HH_EXACT_LAW
heston = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0, strike=100.0, cp=-1.0)
flat = dict(heston, V0=0.0, kappa=0.0, theta=0.0, rho=0.0, sigma=0.2)
jump, q, vg = _ffi.make_jump(0.8, -0.1, 0.15), _ffi.make_qe(0.0, 1), _ffi.make_vg(-0.3, 0.5)
x = math.log(100.0) - 0.6 + 1.2 / 127 * np.arange(128)
vols = 0.22 + 0.05 * np.sin(3.0 * (x - math.log(100.0)))[None, :] + 0.02 * np.arange(16)[:, None] / 15
lv = _ffi.make_localvol(np.linspace(0.05, 0.95, 16), vols, float(x[0]), 1.2 / 127)
ref = C.byref
mh, mf = _ffi.make_model(**heston), _ffi.make_model(**flat)
MON = _ffi.HH_EXTREMES_MONITORED
pay = (_ffi.hh_path_payoff * 1)()
pay[0].kind, pay[0].strike, pay[0].cp = _ffi.HH_PAYOFF_VANILLA, 100.0, -1.0
out1 = (_ffi.hh_result * 1)()

# name -> (kind, model, dynamics, strategy, source structs, the statistics call (c, every))
SOURCES = {
    "euler_lognormal": (_ffi.HH_SOURCE_EULER, mf, GBM, EM, {},
                        lambda c, e: lib.hh_mc_path_stats(h, ref(mf), ref(c), e, 0, stats.data_ptr(), 1, None)),
    "euler_heston": (_ffi.HH_SOURCE_EULER, mh, HES, EM, {},
                     lambda c, e: lib.hh_mc_path_stats(h, ref(mh), ref(c), e, 0, stats.data_ptr(), 1, None)),
    # the jump form has no statistics-only entry point: its solve's first slot is the statistics kernel
    "merton": (_ffi.HH_SOURCE_JUMP, mf, GBM, EM, dict(jump=jump),
               lambda c, e: lib.hh_mc_solve_path_jump(h, ref(mf), ref(jump), ref(c), e, 0, pay, 1, out1, None, None)),
    "qe_martingale": (_ffi.HH_SOURCE_QE, mh, HES, QE, dict(qe=q),
                      lambda c, e: lib.hh_mc_path_stats_qe(h, ref(mh), ref(q), ref(c), e, 0, stats.data_ptr(), 1, None, None)),
    "bates_martingale": (_ffi.HH_SOURCE_BATES, mh, HES, QE, dict(qe=q, jump=jump),
                         lambda c, e: lib.hh_mc_path_stats_bates(h, ref(mh), ref(q), ref(jump), ref(c), e, 0, stats.data_ptr(), 1,
                                                                 None, None)),
    "localvol_16x128": (_ffi.HH_SOURCE_LOCALVOL, mf, GBM, EM, dict(localvol=lv),
                        lambda c, e: lib.hh_mc_path_stats_lv(h, ref(mf), ref(lv), ref(c), e, 0, MON, stats.data_ptr(), 1, None)),
    "variance_gamma": (_ffi.HH_SOURCE_VG, mf, GBM, LAW, dict(vg=vg),
                       lambda c, e: lib.hh_mc_path_stats_vg(h, ref(mf), ref(vg), ref(c), e, 0, stats.data_ptr(), 1, None)),
}
lines = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    lines.append(rec)


def first_slot(call):
    ctx.enable_timing(True)
    ctx.check(call())
    slots = ctx.read_timings()
    ctx.enable_timing(False)
    return slots[0]


def median_of(call, value=first_slot):
    return float(np.median([value(call) for _ in range(args.warmup + args.reps)][args.warmup:]))


def config(dyn, strat, anti):
    c = _ffi.make_config(dyn, strat, n, steps, antithetic=anti, em_split=1)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


ramp = config(HES, EM, 0)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    ctx.check(lib.hh_mc_path_stats(h, ref(mh), ref(ramp), steps, 0, stats.data_ptr(), 1, None))

for run in (1, 2):
    for name, (kind, m, dyn, strat, structs, stats_call) in SOURCES.items():
        source = _ffi.make_path_source(kind, **structs)
        for anti in (0, 1):
            c = config(dyn, strat, anti)
            for every in (steps // 12, 1):
                n_dates = steps // every
                rec = dict(run=run, source=name, antithetic=anti, n=n, steps=steps, dates=n_dates,
                           stats_ms=median_of(lambda: stats_call(c, every)))
                rec["grid_ms"] = median_of(lambda: lib.hh_mc_path_grid(h, ref(source), ref(m), ref(c), every, None, 0, None))
                rec["write_ms"] = 8.0 * n * (1 + anti) * (n_dates + 1) / HBM_RATE * 1e3
                rec["excess_ms"] = rec["grid_ms"] - rec["stats_ms"] - rec["write_ms"]
                res = _ffi.hh_lsm_result()
                D = math.exp(-0.03 * every / steps)

                def lsm():
                    ctx.check(lib.hh_lsm_solve_path(h, ref(source), ref(m), ref(c), every, 3, D, ref(res), None, None, None))
                    return res.kernel_ms
                rec["lsm_kernel_ms"] = median_of(lsm, value=lambda call: call())
                rec["induction_ms"] = rec["lsm_kernel_ms"] - rec["grid_ms"]
                rec["lsm_form"], rec["price"] = res.form, res.price
                emit(rec)

keys = ["stats_ms", "grid_ms", "write_ms", "excess_ms", "lsm_kernel_ms", "induction_ms"]
with open(args.out, "w") as f:
    f.write(f"{'source':<18}{'anti':>5}{'dates':>6}  " + "".join(f"{k + ' r1':>18}{k + ' r2':>18}" for k in keys) + "\n")
    rows = {}
    for r in lines:
        rows.setdefault((r["source"], r["antithetic"], r["dates"]), {})[r["run"]] = r
    for (name, anti, dates), by_run in rows.items():
        f.write(f"{name:<18}{anti:>5}{dates:>6}  " + "".join(f"{by_run[1][k]:>18.4f}{by_run[2][k]:>18.4f}" for k in keys) + "\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print(open(args.out).read().split("\n\n")[0])
