#!/usr/bin/env python3
"""Multilevel Monte Carlo: what the coupled kernel costs and what the coupling buys, in one process and sitting.

  * coupled_stats_kernel (the one timing slot of hh_mc_path_stats_coupled) for Heston, 10^6 trajectories, fine steps 64 and
    252, monitored at expiry only and every 2 fine steps, beside path_stats_kernel (the one slot of hh_mc_path_stats — the
    kernel as it was before the coupled one came: adding the latter left its code unchanged) at the fine step count and at
    the coarse one: running the two legs apart costs the sum of the two.
  * the per-level variances of the mild case of tests/mlmc_cases.py (steps 4 → 32, the tests' trajectories and seed; then
    4 → 64 and 4 → 1024 with 2^14 trajectories on every further level) for the call and the Asian, and from them the cost of
    a multilevel solve over that of a single-level solve on the finest grid AT EQUAL STANDARD ERROR, in steps:
        single level  Var(P_L)·steps_L          multilevel  (Σ_l √(V_l·C_l))²      C_0 = steps_0, C_l = 1.5·steps_l
    (the trajectory counts of either are proportional to 1/ε², which cancels).

Times are the library's own events (hh_ctx_enable_timing): median of `--reps` calls after `--warmup` calls of the same shape,
the table twice; the process first runs solves for about a second so that the clocks have ramped.  The statistics stay in
device memory.  One JSON line per row, and a table at the end.  GPU box only.  (The kernels' register counts are
tools/kernel_regs.py's, read from the objects of the build: `python tools/kernel_regs.py default coupled_stats level_payoff`.)

usage: python tools/mlmc_timing.py [--n 1000000] [--reps 10] [--warmup 3] [--out FILE]"""
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

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import mlmc_cases as mc

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlmc_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n = args.n
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
stats = torch.empty(_ffi.HH_PATH_STATS * 2 * n, dtype=torch.float64, device="cuda")
p = mc.MILD
m = _ffi.make_model(S0=p["S0"], V0=p["V0"], kappa=p["kappa"], theta=p["theta"], sigma=p["sigma"], rho=p["rho"], r=p["r"], T=p["T"])
lines, levels = [], []


def emit(rec, into=lines):
    print(json.dumps(rec), flush=True)
    into.append(rec)


def slot_of(call):
    ctx.enable_timing(True)
    call()
    slots = ctx.read_timings()
    ctx.enable_timing(False)
    assert len(slots) == 1, slots
    return slots[0]


def median_of(call):
    return float(np.median([slot_of(call) for _ in range(args.warmup + args.reps)][args.warmup:]))


def config(steps):
    c = _ffi.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, n, steps, em_split=1)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    return c


def plain(c, every):
    ctx.check(lib.hh_mc_path_stats(h, C.byref(m), C.byref(c), every, 0, stats.data_ptr(), 1, None))


def coupled(c, every):
    ctx.check(lib.hh_mc_path_stats_coupled(h, C.byref(m), C.byref(c), every, 0, stats.data_ptr(), 1, None))


ramp = config(252)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    plain(ramp, 252)

for run in (1, 2):
    for steps in (64, 252):
        for every in (steps, 2):
            cf, cc = config(steps), config(steps // 2)
            both_ms = median_of(lambda: coupled(cf, every))
            fine_ms = median_of(lambda: plain(cf, every))
            coarse_ms = median_of(lambda: plain(cc, every // 2))
            emit(dict(run=run, n=n, fine_steps=steps, monitor_every=every, coupled_ms=round(both_ms, 4), fine_ms=round(fine_ms, 4),
                      coarse_ms=round(coarse_ms, 4), coupled_over_fine=round(both_ms / fine_ms, 3),
                      coupled_over_apart=round(both_ms / (fine_ms + coarse_ms), 3)))

# ---- what the coupling buys: the tests' case, measured ----
market = hh.HestonInputs(hh.Date(2021, 1, 1), p["r"], p["S0"], p["V0"], p["kappa"], p["theta"], p["sigma"], p["rho"])
expiry = hh.Date(2022, 1, 1)
for top in (3, 4, 8):
    counts = mc.TRAJECTORIES + (2 ** 14,) * (top - 3)
    method = hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.MLMCConfig(mc.STEPS0, trajectories=counts, seed=7))
    finest = mc.STEPS0 << top
    single = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(2 ** 18, steps=finest, seeds=np.arange(1, 2 ** 18 + 1)))
    for name, payoff, payoff_single in (
            ("call",) + (hh.VanillaOption(p["K"], expiry, hh.European(), hh.Call(), hh.Spot()),) * 2,
            ("asian", hh.AsianOption(p["K"], expiry, hh.Call(), hh.ArithmeticAverage(), hh.Monitoring(1)),
             hh.AsianOption(p["K"], expiry, hh.Call(), hh.ArithmeticAverage(), hh.Monitoring(finest // mc.DATES)))):
        ml = hh.solve(hh.PricingProblem(payoff, market), method)
        sl = hh.solve(hh.PricingProblem(payoff_single, market), single, ensemble=False)
        V = [lv.variance for lv in ml.levels]
        var_single = sl.std_error ** 2 * 2 ** 18
        cost_ml = sum(math.sqrt(v * method.config.level_cost(l)) for l, v in enumerate(V)) ** 2
        emit(dict(payoff=name, steps=[lv.steps for lv in ml.levels], trajectories=list(counts), variances=[round(v, 5) for v in V],
                  means=[round(lv.mean, 5) for lv in ml.levels], price=round(ml.price, 5), std_error=round(ml.std_error, 5),
                  single_level_price=round(sl.price, 5), single_level_variance=round(var_single, 4),
                  single_over_multilevel_cost=round(var_single * finest / cost_ml, 3)), levels)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(f"Multilevel Monte Carlo: the coupled statistics kernel beside the two plain ones, and what the coupling buys "
            f"(tools/mlmc_timing.py); library {os.path.basename(_ffi.LIB_PATH)}\n"
            f"median of {args.reps} calls after {args.warmup} warm-up calls, ms by the library's events; two runs in one sitting\n"
            f"Heston kappa {p['kappa']}, theta = V0 = {p['V0']}, sigma {p['sigma']}, rho {p['rho']}, r {p['r']}, T {p['T']}\n\n")
    f.write(f"{'run':>3} {'shape':>15} {'every':>5} | {'coupled':>9} {'fine':>9} {'coarse':>9} {'/fine':>6} {'/apart':>6}\n")
    for r in lines:
        f.write(f"{r['run']:>3} {str(r['n']) + ' x ' + str(r['fine_steps']):>15} {r['monitor_every']:>5} | {r['coupled_ms']:>9.4f} "
                f"{r['fine_ms']:>9.4f} {r['coarse_ms']:>9.4f} {r['coupled_over_fine']:>6.3f} {r['coupled_over_apart']:>6.3f}\n")
    f.write("\nper-level variances (discounted) and the cost of a single-level solve on the finest grid over the multilevel one, "
            "at equal standard error\n")
    for r in levels:
        f.write(f"{r['payoff']:>6} steps {r['steps'][0]} -> {r['steps'][-1]:>4}: V = {r['variances']}  single-level variance "
                f"{r['single_level_variance']}  cost ratio {r['single_over_multilevel_cost']}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines + levels) + "\n")
print("wrote", args.out)
