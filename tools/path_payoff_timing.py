#!/usr/bin/env python3
"""Path-dependent payoffs (hh_mc_solve_path) for Heston H252, 10^6 trajectories x 252 steps, with and without
antithetic, monitored daily (every step), monthly (every 21 steps) and at expiry alone — beside, in the same process
and sitting, the European GENERATE solve (hh_mc_solve) and the spot grid (hh_euler_grid) of the same configuration,
whose draws and steps the statistics kernel repeats.  The same for lognormal dynamics (sigma 0.2), and for each row
the BRIDGE form of the statistics kernel (hh_mc_path_stats_ex, HH_EXTREMES_BRIDGE: seven rows, the continuous extremes
over every step whatever the monitoring), left on the device.

Times are the library's own events: the two timing slots of a call (hh_ctx_enable_timing: the statistics kernel; the
payoff kernel with its record reduction) and kernel_ms of the whole call (seeds already on the device, so the window
holds the upload of the payoffs and the kernels).  Median of `--reps` calls after `--warmup` calls of the same shape;
the process first runs European solves for about a second so that the clocks have ramped before anything is timed.
One JSON line per configuration, and a table at the end.  GPU box only.

usage: python tools/path_payoff_timing.py [--n 1000000] [--steps 252] [--reps 10] [--warmup 3] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_payoff_timing.txt"))
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
m_heston = _ffi.make_model(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0, strike=100.0, cp=1.0)
m_logn = _ffi.make_model(S0=100.0, sigma=0.2, r=0.03, T=1.0, strike=100.0, cp=1.0)
m = m_heston


def payoff(kind, strike=100.0, cp=1.0, barrier_type=0, barrier=0.0, rebate=0.0, cash=0.0):
    q = _ffi.hh_path_payoff()
    q.kind, q.barrier_type, q.strike, q.cp, q.barrier, q.rebate, q.cash = kind, barrier_type, strike, cp, barrier, rebate, cash
    return q


# 16 payoffs: four of each family, strikes spread around the money
SIXTEEN = [payoff(_ffi.HH_PAYOFF_ASIAN_ARITH, 90.0 + 5.0 * k, 1.0 if k % 2 else -1.0) for k in range(4)] + \
          [payoff(_ffi.HH_PAYOFF_ASIAN_GEOM, 90.0 + 5.0 * k, 1.0 if k % 2 else -1.0) for k in range(4)] + \
          [payoff(_ffi.HH_PAYOFF_BARRIER, 100.0, 1.0, t, 120.0 if t < 2 else 85.0, 1.0) for t in range(4)] + \
          [payoff(_ffi.HH_PAYOFF_DIGITAL_CASH, 100.0, 1.0, cash=1.0), payoff(_ffi.HH_PAYOFF_DIGITAL_ASSET, 100.0, -1.0),
           payoff(_ffi.HH_PAYOFF_VANILLA, 100.0, 1.0), payoff(_ffi.HH_PAYOFF_VANILLA, 100.0, -1.0)]


def median_of(call):
    rows = [call() for _ in range(args.warmup + args.reps)][args.warmup:]
    return [float(np.median([r[i] for r in rows])) for i in range(len(rows[0]))]


lines = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    lines.append(rec)


# clock ramp: European solves for about a second
ramp = _ffi.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, n, steps)
ramp.seeds, ramp.seeds_on_device, ramp.seeds_len = seeds.data_ptr(), 1, n
res = _ffi.hh_result()
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:
    ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(ramp), C.byref(res), None))

for name, dyn, m in (("heston", _ffi.HH_HESTON, m_heston), ("lognormal", _ffi.HH_LOGNORMAL, m_logn)):
    for anti in (0, 1):
        c = _ffi.make_config(dyn, _ffi.HH_EULER_MARUYAMA, n, steps, antithetic=anti)
        c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
        ntot = n * (2 if anti else 1)

        def european():
            ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(c), C.byref(res), None))
            return (res.kernel_ms,)

        spot = torch.empty((steps + 1) * ntot, dtype=torch.float64, device="cuda")

        def grid():
            ctx.check(lib.hh_euler_grid(h, C.byref(m), C.byref(c), _ffi.HH_PATH_SPOT, spot.data_ptr(), None, 1, C.byref(res)))
            return (res.kernel_ms,)

        (eu_ms,), (grid_ms,) = median_of(european), median_of(grid)
        del spot
        emit(dict(what="reference", dynamics=name, antithetic=anti, n=n, steps=steps, european_generate_ms=round(eu_ms, 4),
                  spot_grid_ms=round(grid_ms, 4)))
        for every in (1, 21, steps):
            if steps % every:
                continue
            row = dict(what="path", dynamics=name, antithetic=anti, n=n, steps=steps, monitor_every=every)
            for K in (1, 16):
                arr, out = (_ffi.hh_path_payoff * K)(*SIXTEEN[:K]), (_ffi.hh_result * K)()

                def solve():
                    ctx.enable_timing(True)
                    ctx.check(lib.hh_mc_solve_path(h, C.byref(m), C.byref(c), every, 0, arr, K, out, None, None))
                    slots = ctx.read_timings()
                    ctx.enable_timing(False)
                    assert len(slots) == 2, slots
                    return slots[0], slots[1], out[0].kernel_ms, out[0].total_ms

                s_ms, p_ms, k_ms, w_ms = median_of(solve)
                row.update({f"stats_kernel_ms_K{K}": round(s_ms, 4), f"payoff_kernels_ms_K{K}": round(p_ms, 4),
                            f"call_kernel_ms_K{K}": round(k_ms, 4), f"call_wall_ms_K{K}": round(w_ms, 4)})
            seven = torch.empty(_ffi.HH_PATH_STATS_BRIDGE * ntot, dtype=torch.float64, device="cuda")

            def bridge():
                ctx.enable_timing(True)
                ctx.check(lib.hh_mc_path_stats_ex(h, C.byref(m), C.byref(c), every, 0, _ffi.HH_EXTREMES_BRIDGE,
                                                  seven.data_ptr(), 1, C.byref(res)))
                slots = ctx.read_timings()
                ctx.enable_timing(False)
                assert len(slots) == 1, slots
                return (slots[0],)

            (b_ms,) = median_of(bridge)
            del seven
            row["bridge_stats_kernel_ms"] = round(b_ms, 4)
            row["bridge_vs_stats"] = round(b_ms / row["stats_kernel_ms_K1"], 4)
            row["stats_vs_european"] = round(row["stats_kernel_ms_K1"] / eu_ms, 4)
            row["stats_vs_spot_grid"] = round(row["stats_kernel_ms_K1"] / grid_ms, 4)
            row["path_steps_per_s"] = round(n * steps / (row["call_kernel_ms_K1"] * 1e-3), 0)
            emit(row)

with open(args.out, "w") as f:
    f.write(f"Path-dependent payoffs (hh_mc_solve_path, hh_mc_path_stats_ex): Heston H252 and lognormal, {n} trajectories x "
            f"{steps} steps; library {os.path.basename(_ffi.LIB_PATH)}\nmedian of {args.reps} calls after {args.warmup} warm-up calls, ms by the "
            "library's events (tools/path_payoff_timing.py)\n\n")
    f.write(f"{'dynamics':>9} {'anti':>4} {'every':>5} | {'European':>9} {'spot grid':>9} | {'stats':>8} {'pay K=1':>8} {'call K=1':>8} "
            f"{'pay K=16':>8} {'call K=16':>9} | {'stats/Eur':>9} {'stats/grid':>10} | {'bridge':>8} {'bridge/stats':>12}\n")
    ref = {}
    for r in lines:
        if r["what"] == "reference":
            ref[r["dynamics"], r["antithetic"]] = r
            continue
        e = ref[r["dynamics"], r["antithetic"]]
        f.write(f"{r['dynamics']:>9} {r['antithetic']:>4} {r['monitor_every']:>5} | {e['european_generate_ms']:>9.4f} {e['spot_grid_ms']:>9.4f} | "
                f"{r['stats_kernel_ms_K1']:>8.4f} {r['payoff_kernels_ms_K1']:>8.4f} {r['call_kernel_ms_K1']:>8.4f} "
                f"{r['payoff_kernels_ms_K16']:>8.4f} {r['call_kernel_ms_K16']:>9.4f} | {r['stats_vs_european']:>9.4f} "
                f"{r['stats_vs_spot_grid']:>10.4f} | {r['bridge_stats_kernel_ms']:>8.4f} {r['bridge_vs_stats']:>12.4f}\n")
    f.write("\n" + "\n".join(json.dumps(r) for r in lines) + "\n")
print("wrote", args.out)
