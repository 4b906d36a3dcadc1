#!/usr/bin/env python3
"""The state rows of the several-asset walk beside its statistics kernel, and the several-variable LSM induction beside the
one-variable one, in the same process and sitting:

  * assets_rows_kernel — the one timing slot of hh_assets_path_rows — at d = 1, 2, 4, 8 on 12 and `steps` dates, plain,
    beside assets_stats_kernel (geometric index; the slot of hh_mc_path_stats_assets) at the same d and dates.  The
    expectation it is held against: statistics + the time to write 8·d·n_total·(n_dates + 1) bytes at 6.99 TB/s, the rate
    README's headline reaches.  `excess_ms` is what the rows take beyond that (negative: inside it);
  * the induction on those rows (hh_lsm_solve_states on a device grid, a worst-of put) at (m, p) = (2, 3), (4, 2), (8, 2) on
    12 dates: kernel_ms and the time per date, beside hh_lsm_solve_grid's launch-per-date form (HH_OPT_LSM_FORM) on one row
    of spots — the index of the same trajectories — at degree 3.  `gram_bytes_ms` is 8·m·n_total bytes per regressed date
    at the HBM rate: what the Gram pass would cost were it bound by memory.  The pass's share of the induction is read
    from a kernel trace of `--induction-only` (rocprofv3 --kernel-trace --stats -- python tools/assets_lsm_timing.py
    --induction-only): multi_gram_kernel's total beside the other kernels'.

Times are the library's own events.  Median of `--reps` calls after `--warmup`, the table twice (two runs: their
difference is the spread), after a second of solves so that the clocks have ramped.  One JSON line per row, printed and
written to --out (profiles/assets_lsm_timing_table.txt, which profiles/assets_lsm_timing.txt quotes).  GPU box only.

usage: python tools/assets_lsm_timing.py [--n 1000000] [--steps 252] [--reps 5] [--warmup 2] [--out FILE]"""
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
ap.add_argument("--induction-only", action="store_true", help="one run of the inductions alone (for a kernel trace)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assets_lsm_timing_table.txt"))
args = ap.parse_args()

HBM_RATE = 6.99e12
ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
ref = C.byref
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS * n, dtype=torch.float64, device="cuda")
model = _ffi.make_model(S0=1.0, V0=0.0, kappa=0.0, theta=0.0, sigma=0.0, rho=0.0, r=0.03, T=1.0, strike=100.0, cp=-1.0)
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


def assets(d, kind):
    corr = [[0.5 ** abs(i - j) for j in range(d)] for i in range(d)]
    w = [1.0] * d if kind in (_ffi.HH_INDEX_BEST_OF, _ffi.HH_INDEX_WORST_OF) else [1.0 / d] * d
    return _ffi.make_assets([100.0] * d, [0.2 + 0.02 * i for i in range(d)], w, corr, kind)


def config():
    c = _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, n, steps)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


c = config()
ramp = assets(2, _ffi.HH_INDEX_GEOMETRIC)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    ctx.check(lib.hh_mc_path_stats_assets(h, ref(model), ref(ramp), ref(c), steps, 0, stats.data_ptr(), 1, None))

for run in ((1,) if args.induction_only else (1, 2)):
    for d in (() if args.induction_only else (1, 2, 4, 8)):
        geo = assets(d, _ffi.HH_INDEX_GEOMETRIC)
        for every in (steps // 12, 1):
            n_dates = steps // every
            rows = torch.empty(lib.hh_assets_rows_elems(n, n_dates, d, 0), dtype=torch.float64, device="cuda")
            rec = dict(run=run, what="rows", d=d, n=n, steps=steps, dates=n_dates,
                       stats_ms=median_of(lambda: lib.hh_mc_path_stats_assets(h, ref(model), ref(geo), ref(c), every, 0,
                                                                              stats.data_ptr(), 1, None)),
                       rows_ms=median_of(lambda: lib.hh_assets_path_rows(h, ref(model), ref(geo), ref(c), every, rows.data_ptr(), 1,
                                                                         None)))
            rec["write_ms"] = 8.0 * d * n * (n_dates + 1) / HBM_RATE * 1e3
            rec["excess_ms"] = rec["rows_ms"] - rec["stats_ms"] - rec["write_ms"]
            emit(rec)
            del rows
    # the inductions, on 12 dates (16 GB of rows at d = 8 and 252 dates do not leave room for a second grid)
    every, n_dates = steps // 12, 12
    D = math.exp(-0.03 * every / steps)
    for m, p in ((2, 3), (4, 2), (8, 2)):
        worst = assets(m, _ffi.HH_INDEX_WORST_OF)
        rows = torch.empty(lib.hh_assets_rows_elems(n, n_dates, m, 0), dtype=torch.float64, device="cuda")
        ctx.check(lib.hh_assets_path_rows(h, ref(model), ref(worst), ref(c), every, rows.data_ptr(), 1, None))
        res = _ffi.hh_lsm_result()

        def solve(strike):
            desc = _ffi.hh_lsm_states()
            desc.kind, desc.n_states, desc.index_kind, desc.cp, desc.strike = _ffi.HH_LSM_STATES_LOG_ASSETS, m, _ffi.HH_INDEX_WORST_OF, -1.0, strike
            for i in range(m):
                desc.weights[i] = 1.0

            def call():
                ctx.check(lib.hh_lsm_solve_states(h, ref(desc), rows.data_ptr(), n, n_dates, p, D, ref(res), None, None, None))
                return res.kernel_ms
            return median_of(call, value=lambda f: f())

        total = solve(100.0)
        rec = dict(run=run, what="induction", m=m, p=p, B=math.comb(m + p, p), n=n, dates=n_dates, induction_ms=total,
                   per_date_us=1e3 * total / n_dates, rows_regressed=res.rows_regressed, price=res.price,
                   gram_bytes_ms=8.0 * m * n * (n_dates - 1) / HBM_RATE * 1e3)
        emit(rec)
        if m == 2:   # the one-variable induction, launch per date, on the index row of the same trajectories
            index = torch.exp(torch.minimum(rows.view(n_dates + 1, m, n)[:, 0], rows.view(n_dates + 1, m, n)[:, 1])).contiguous()
            m1 = _ffi.make_model(S0=100.0, sigma=0.2, r=0.03, T=1.0, strike=100.0, cp=-1.0)
            ctx.check(lib.hh_ctx_set_option(h, _ffi.HH_OPT_LSM_FORM, _ffi.HH_LSM_FORM_PER_DATE))

            def one():
                ctx.check(lib.hh_lsm_solve_grid(h, ref(m1), index.data_ptr(), n, n_dates, 3, D, ref(res), None, None))
                return res.kernel_ms
            t = median_of(one, value=lambda f: f())
            ctx.check(lib.hh_ctx_set_option(h, _ffi.HH_OPT_LSM_FORM, _ffi.HH_LSM_FORM_AUTO))
            emit(dict(run=run, what="one-variable", n=n, dates=n_dates, degree=3, induction_ms=t, per_date_us=1e3 * t / n_dates,
                      price=res.price))
        del rows

with open(args.out + (".induction_only" if args.induction_only else ""), "w") as f:
    f.write("\n".join(json.dumps(r) for r in lines) + "\n")
print(f"wrote {args.out}")
