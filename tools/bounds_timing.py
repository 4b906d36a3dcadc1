#!/usr/bin/env python3
"""The dual upper bound's nested kernel beside the path-statistics kernel it shares its step with, and the forward valuation
beside the time to read its rows, in the same process and sitting:

  * nested_continuation_kernel (hh_lsm_upper_bound's nested_ms) at `--outer` columns × 12 dates × `--inner` walks × `--steps`
    steps under the never-exercise policy (every walk runs to expiry) and under a fitted policy (walks stop early, waves leave
    when all 64 have), as inner path-steps per second — counting, for both, the steps of walks that run to expiry;
  * path_stats_kernel<HestonModel> (the timing slot of hh_mc_path_stats) on the same number of path-steps in one launch of
    full-length walks, and the ratio.  The nested kernel cannot exceed it: the same step, plus a policy evaluation per date;
  * policy_value_kernel (the timing slot of hh_lsm_policy_value, with the final Σ kernel) on `--n` columns × 12 dates against
    the time to read its 16·n·12 bytes of rows once at 6.99 TB/s, README's headline rate.

Times are the library's own events; median of `--reps` calls after `--warmup`, after a second of solves.  One JSON line per
row, printed and written to --out.  GPU box only.

usage: python tools/bounds_timing.py [--outer 4096] [--inner 256] [--steps 48] [--n 1000000] [--reps 7] [--warmup 2] [--out FILE]"""
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
ap.add_argument("--outer", type=int, default=4096)
ap.add_argument("--inner", type=int, default=256)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounds_timing_table.txt"))
args = ap.parse_args()

HBM_RATE = 6.99e12  # bytes/s: README's headline
DATES, DEGREE = 12, 3
ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
ref = C.byref
steps, every = args.steps, args.steps // DATES
B = math.comb(2 + DEGREE, DEGREE)
# DESIGN §5.22's case: the policy exercises early on a good share of the walks
m = _ffi.make_model(S0=100.0, V0=0.16, kappa=0.5, theta=0.16, sigma=1.5, rho=0.0, r=0.05, T=2.0, strike=100.0, cp=-1.0)
D = math.exp(-m.r_drift * m.T * every / steps)
euler = _ffi.make_path_source(_ffi.HH_SOURCE_EULER)
lines = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    lines.append(rec)


def config(n, first=1):
    c = _ffi.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, n, steps, seeds=np.arange(first, first + n, dtype=np.uint64))
    return c


def median(values):
    return float(np.median(values[args.warmup:]))


def slot(call):
    ctx.enable_timing(True)
    ctx.check(call())
    slots = ctx.read_timings()
    ctx.enable_timing(False)
    return slots


# the policies: fitted on 200 000 columns, and never-exercise
fit_cfg = config(200_000)
fitted = np.empty((DATES + 1, 4 + B))
res = _ffi.hh_lsm_result()
ctx.check(lib.hh_lsm_fit_path_states(h, ref(euler), ref(m), ref(fit_cfg), every, DEGREE, D, ref(res), fitted.ctypes.data))
never = np.zeros((DATES + 1, 4 + B))
never[:, 2:4], never[:, 4] = 1.0, 1e300

# full-length walks of the same number of path-steps for the statistics kernel
inner_steps = sum(args.outer * args.inner * (steps - every * t) for t in range(DATES))
n_stats = inner_steps // steps
stats_cfg = config(n_stats)
stats_buf = torch.empty(_ffi.HH_PATH_STATS * n_stats, dtype=torch.float64, device="cuda")
stats_call = lambda: lib.hh_mc_path_stats(h, ref(m), ref(stats_cfg), every, 0, stats_buf.data_ptr(), 1, None)  # noqa: E731

t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    ctx.check(stats_call())

outer_cfg = config(args.outer, first=10_000_001)
out = _ffi.hh_bounds_result()
for run in (1, 2):
    t_stats = median([slot(stats_call)[0] for _ in range(args.warmup + args.reps)])
    rec = dict(run=run, what="nested", outer=args.outer, dates=DATES, inner=args.inner, steps=steps, inner_path_steps=inner_steps,
               stats_paths=n_stats, stats_ms=t_stats, stats_path_steps_per_s=n_stats * steps / (t_stats * 1e-3))
    for name, policy in (("never", never), ("fitted", fitted)):
        t, dual = [], []
        for _ in range(args.warmup + args.reps):
            ctx.check(lib.hh_lsm_upper_bound(h, ref(m), ref(outer_cfg), every, policy.ctypes.data, DEGREE, D, args.inner, 7, ref(out),
                                             None, None, None))
            t.append(out.nested_ms)
            dual.append(out.outer_ms)
        rec[name + "_nested_ms"] = median(t)
        rec[name + "_path_steps_per_s"] = inner_steps / (median(t) * 1e-3)
        rec[name + "_ratio_to_stats"] = t_stats / median(t)
        rec[name + "_outer_ms"] = median(dual)
        rec[name + "_upper"] = out.upper
    emit(rec)

    # the forward valuation on n columns
    n = args.n
    val_cfg = config(n, first=20_000_001)
    rows = torch.empty(lib.hh_assets_rows_elems(n, DATES, 2, 0), dtype=torch.float64, device="cuda")
    ctx.check(lib.hh_mc_path_states(h, ref(euler), ref(m), ref(val_cfg), every, rows.data_ptr(), 1, None))
    desc = _ffi.hh_lsm_states()
    desc.kind, desc.n_states, desc.cp, desc.strike = _ffi.HH_LSM_STATES_LOG_SPOT_VARIANCE, 2, -1.0, 100.0
    rec = dict(run=run, what="forward", n=n, dates=DATES, read_ms=16.0 * n * DATES / HBM_RATE * 1e3)
    for name, policy in (("never", never), ("fitted", fitted)):
        call = lambda: lib.hh_lsm_policy_value(h, ref(desc), policy.ctypes.data, DEGREE, rows.data_ptr(), n, DATES, D, ref(res),  # noqa: E731
                                               None, None)
        rec[name + "_ms"] = median([slot(call)[0] for _ in range(args.warmup + args.reps)])
        rec[name + "_over_read"] = rec[name + "_ms"] / rec["read_ms"]
        rec[name + "_price"] = res.price
    emit(rec)
    del rows

with open(args.out, "w") as f:
    f.write("\n".join(json.dumps(r) for r in lines) + "\n")
