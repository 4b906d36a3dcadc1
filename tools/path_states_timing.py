#!/usr/bin/env python3
"""The state-row form (log S, V) of the stochastic-volatility walks beside its date-row and statistics siblings, and the
(S, V) induction beside the two-asset one, in the same process and sitting:

  * per source (Heston Euler, QE and Bates with the martingale correction) the statistics kernel — the one timing slot of
    the source's hh_mc_path_stats* call — at monitor_every = e, the date-row kernel — the slot of hh_mc_path_grid — and the
    state-row kernel — the slot of hh_mc_path_states — at exercise_every = e, for e = steps/12 and e = 1 (12 and `steps`
    dates), plain and antithetic.  The expectation the state rows are held against: statistics + the time to write
    16·n_total·(n_dates + 1) bytes at 6.99 TB/s, the rate README's headline reaches.  `excess_ms` is what the state rows
    take beyond that (negative: inside it);
  * the induction at degree 3 (B = 10) on 12 dates of n columns: hh_lsm_solve_states under
    HH_LSM_STATES_LOG_SPOT_VARIANCE on the Heston Euler walk's rows, and under HH_LSM_STATES_LOG_ASSETS (a worst-of put, d = 2:
    what hh_lsm_solve_assets runs) on hh_assets_path_rows' rows, ALTERNATING call by call; kernel_ms and the time per date
    of each, and their ratio.  THE BAR: the ratio is at most 1.05.

Times are the library's own events.  Median of `--reps` calls after `--warmup`, the table twice (two runs: their difference
is the spread), after a second of solves so that the clocks have ramped.  One JSON line per row, printed and written to
--out (profiles/path_states_timing_table.txt, which profiles/path_states_timing.txt quotes beside what no tool writes: the
disassembly comparison and the register report).  GPU box only.

usage: python tools/path_states_timing.py [--n 1000000] [--steps 252] [--reps 5] [--warmup 2] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_states_timing_table.txt"))
args = ap.parse_args()

HBM_RATE = 6.99e12  # bytes/s: README's headline
ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
ref = C.byref
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS * 2 * n, dtype=torch.float64, device="cuda")
rows_buf = torch.empty(lib.hh_assets_rows_elems(n, steps, 2, 1), dtype=torch.float64, device="cuda")
HES, EM, QE = _ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, _ffi.HH_QE
mh = _ffi.make_model(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0, strike=100.0, cp=-1.0)
jump, q = _ffi.make_jump(0.8, -0.1, 0.15), _ffi.make_qe(0.0, 1)

# name -> (kind, strategy, source structs, the statistics call (c, every))
SOURCES = {
    "euler_heston": (_ffi.HH_SOURCE_EULER, EM, {},
                     lambda c, e: lib.hh_mc_path_stats(h, ref(mh), ref(c), e, 0, stats.data_ptr(), 1, None)),
    "qe_martingale": (_ffi.HH_SOURCE_QE, QE, dict(qe=q),
                      lambda c, e: lib.hh_mc_path_stats_qe(h, ref(mh), ref(q), ref(c), e, 0, stats.data_ptr(), 1, None, None)),
    "bates_martingale": (_ffi.HH_SOURCE_BATES, QE, dict(qe=q, jump=jump),
                         lambda c, e: lib.hh_mc_path_stats_bates(h, ref(mh), ref(q), ref(jump), ref(c), e, 0, stats.data_ptr(), 1,
                                                                 None, None)),
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
    for name, (kind, strat, structs, stats_call) in SOURCES.items():
        source = _ffi.make_path_source(kind, **structs)
        for anti in (0, 1):
            c = config(HES, strat, anti)
            for every in (steps // 12, 1):
                n_dates = steps // every
                rec = dict(run=run, what="rows", source=name, antithetic=anti, n=n, steps=steps, dates=n_dates,
                           stats_ms=median_of(lambda: stats_call(c, every)),
                           date_rows_ms=median_of(lambda: lib.hh_mc_path_grid(h, ref(source), ref(mh), ref(c), every, None, 0, None)),
                           state_rows_ms=median_of(lambda: lib.hh_mc_path_states(h, ref(source), ref(mh), ref(c), every,
                                                                                 rows_buf.data_ptr(), 1, None)))
                rec["write_ms"] = 16.0 * n * (1 + anti) * (n_dates + 1) / HBM_RATE * 1e3
                rec["excess_ms"] = rec["state_rows_ms"] - rec["stats_ms"] - rec["write_ms"]
                emit(rec)

    # the two inductions at (m = 2, degree 3) on 12 dates of n columns, call by call in turn
    every, n_dates, degree = steps // 12, 12, 3
    D = math.exp(-0.03 * every / steps)
    c = config(HES, EM, 0)
    euler = _ffi.make_path_source(_ffi.HH_SOURCE_EULER)
    n_rows = lib.hh_assets_rows_elems(n, n_dates, 2, 0)
    sv_rows = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    ctx.check(lib.hh_mc_path_states(h, ref(euler), ref(mh), ref(c), every, sv_rows.data_ptr(), 1, None))
    two = _ffi.make_assets([100.0, 100.0], [0.2, 0.22], [1.0, 1.0], [[1.0, 0.5], [0.5, 1.0]], _ffi.HH_INDEX_WORST_OF)
    ma = _ffi.make_model(S0=1.0, V0=0.0, kappa=0.0, theta=0.0, sigma=0.0, rho=0.0, r=0.03, T=1.0, strike=100.0, cp=-1.0)
    ca = config(_ffi.HH_LOGNORMAL, EM, 0)
    as_rows = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    ctx.check(lib.hh_assets_path_rows(h, ref(ma), ref(two), ref(ca), every, as_rows.data_ptr(), 1, None))
    d_sv, d_as = _ffi.hh_lsm_states(), _ffi.hh_lsm_states()
    d_sv.kind, d_sv.n_states, d_sv.cp, d_sv.strike = _ffi.HH_LSM_STATES_LOG_SPOT_VARIANCE, 2, -1.0, 100.0
    d_as.kind, d_as.n_states, d_as.index_kind, d_as.cp, d_as.strike = _ffi.HH_LSM_STATES_LOG_ASSETS, 2, _ffi.HH_INDEX_WORST_OF, -1.0, 100.0
    d_as.weights[0] = d_as.weights[1] = 1.0
    res_sv, res_as = _ffi.hh_lsm_result(), _ffi.hh_lsm_result()
    t_sv, t_as = [], []
    for _ in range(args.warmup + 2 * args.reps):
        ctx.check(lib.hh_lsm_solve_states(h, ref(d_sv), sv_rows.data_ptr(), n, n_dates, degree, D, ref(res_sv), None, None, None))
        t_sv.append(res_sv.kernel_ms)
        ctx.check(lib.hh_lsm_solve_states(h, ref(d_as), as_rows.data_ptr(), n, n_dates, degree, D, ref(res_as), None, None, None))
        t_as.append(res_as.kernel_ms)
    sv, two_assets = float(np.median(t_sv[args.warmup:])), float(np.median(t_as[args.warmup:]))
    emit(dict(run=run, what="induction", m=2, degree=degree, B=10, n=n, dates=n_dates, spot_variance_ms=sv,
              spot_variance_per_date_us=1e3 * sv / n_dates, two_assets_ms=two_assets, two_assets_per_date_us=1e3 * two_assets / n_dates,
              ratio=sv / two_assets, within_the_bar=bool(sv <= 1.05 * two_assets), rows_regressed=res_sv.rows_regressed,
              price_spot_variance=res_sv.price, price_two_assets=res_as.price))
    del sv_rows, as_rows

keys = ["stats_ms", "date_rows_ms", "state_rows_ms", "write_ms", "excess_ms"]
with open(args.out, "w") as f:
    f.write(f"{'source':<18}{'anti':>5}{'dates':>6}  " + "".join(f"{k + ' r1':>18}{k + ' r2':>18}" for k in keys) + "\n")
    table = {}
    for r in lines:
        if r["what"] == "rows":
            table.setdefault((r["source"], r["antithetic"], r["dates"]), {})[r["run"]] = r
    for (name, anti, dates), by_run in table.items():
        f.write(f"{name:<18}{anti:>5}{dates:>6}  " + "".join(f"{by_run[1][k]:>18.4f}{by_run[2][k]:>18.4f}" for k in keys) + "\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print(open(args.out).read().split("\n\n")[0])
bad = [r for r in lines if r["what"] == "induction" and not r["within_the_bar"]]
sys.exit(1 if bad else 0)
