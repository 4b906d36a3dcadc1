#!/usr/bin/env python3
"""Euler path grid and LSM on it (hh_euler_grid, hh_lsm_solve_euler) for Heston H252, 10^6 trajectories x 100
dates, with and without antithetic — beside the European GENERATE solve of the same configuration (hh_mc_solve),
whose draws and steps the grid kernel repeats.  Event times (kernel_ms of each call: the seeds are already on the
device, so the window holds the kernels alone) as the median of `--reps` calls after two warm-up calls, wall time
of hh_lsm_solve_euler, the log-state grid (no exp per row), and path-steps/s = trajectories x steps / kernel time (antithetic: the mirrored paths are not
counted, as for the European figures).  One JSON line per configuration.  GPU box only.

usage: python tools/lsm_euler_timing.py [--n 1000000] [--steps 100] [--reps 10] [--degree 5]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hedgehog_jl_amd import _ffi

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--degree", type=int, default=5)
args = ap.parse_args()

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = args.n, args.steps
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
m = _ffi.make_model(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0, strike=100.0,
                    cp=-1.0)
D = math.exp(-0.03 / steps)


def median_ms(call, reps):
    ks, ws = [], []
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        k = call()
        ws.append((time.perf_counter() - t0) * 1e3)
        ks.append(k)
    return float(np.median(ks[2:])), float(np.median(ws[2:]))


for anti in (0, 1):
    c = _ffi.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, n, steps, antithetic=anti)
    c.seeds, c.seeds_on_device, c.seeds_len = seeds.data_ptr(), 1, n
    ntot = n * (2 if anti else 1)
    spot = torch.empty((steps + 1) * ntot, dtype=torch.float64, device="cuda")
    var = torch.empty_like(spot)
    res, lres = _ffi.hh_result(), _ffi.hh_lsm_result()

    def european():
        ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(c), C.byref(res), None))
        return res.kernel_ms

    def grid(with_var, state=_ffi.HH_PATH_SPOT):
        ctx.check(lib.hh_euler_grid(h, C.byref(m), C.byref(c), state, spot.data_ptr(),
                                    var.data_ptr() if with_var else None, 1, C.byref(res)))
        return res.kernel_ms

    def lsm():
        ctx.check(lib.hh_lsm_solve_euler(h, C.byref(m), C.byref(c), _ffi.HH_PATH_SPOT, args.degree, D,
                                         C.byref(lres), None, None, None))
        return lres.kernel_ms

    eu_ms, _ = median_ms(european, args.reps)
    g_ms, _ = median_ms(lambda: grid(False), args.reps)
    gv_ms, _ = median_ms(lambda: grid(True), args.reps)
    gl_ms, _ = median_ms(lambda: grid(False, _ffi.HH_PATH_LOG), args.reps)  # no exp per row: what the exp costs
    l_ms, l_wall = median_ms(lsm, args.reps)
    # the last spot row is the European terminal sample: one check that the grid is what it claims
    term = torch.empty(ntot, dtype=torch.float64, device="cuda")
    c.terminal_on_device = 1
    ctx.check(lib.hh_mc_solve(h, C.byref(m), C.byref(c), C.byref(res), C.c_void_p(term.data_ptr())))
    c.terminal_on_device = 0
    grid(False)
    torch.cuda.synchronize()
    same = bool(torch.equal(spot[steps * ntot:], term))
    rate = lambda ms: n * steps / (ms * 1e-3)
    print(json.dumps({
        "n": n, "steps": steps, "antithetic": anti, "degree": args.degree,
        "european_generate_ms": round(eu_ms, 4), "european_path_steps_per_s": f"{rate(eu_ms):.3e}",
        "grid_ms": round(g_ms, 4), "grid_path_steps_per_s": f"{rate(g_ms):.3e}",
        "grid_over_european_rate": round(eu_ms / g_ms, 3),
        "grid_with_variance_ms": round(gv_ms, 4), "grid_log_state_ms": round(gl_ms, 4),
        "grid_write_GBps": round(8 * ntot * (steps + 1) / (g_ms * 1e-3) / 1e9, 1),
        "lsm_solve_ms": round(l_ms, 4), "lsm_solve_wall_ms": round(l_wall, 4), "lsm_form": lres.form,
        "lsm_price": lres.price, "lsm_std_error": lres.std_error,
        "last_row_is_the_terminal": same}), flush=True)
