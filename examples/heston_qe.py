#!/usr/bin/env python3
"""Heston where the Feller condition fails by far (κ = 0.3, θ = v₀ = 0.04, σ = 0.9, ρ = −0.5, five years): calls at three
strikes by Euler–Maruyama with a clipped variance and by Andersen's quadratic-exponential scheme on 8, 16 and 32 steps
of the same seeds, against Carr–Madan; then a quarterly Asian and a down-and-out call from one QE simulation
(hh_mc_solve_path_qe).  Needs an MI355X."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
expiry = hh.add_years(ref, 5)
market = hh.HestonInputs(ref, 0.0, 100.0, 0.04, 0.3, 0.04, 0.9, -0.5)
strikes = [70.0, 100.0, 140.0]
calls = [hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()) for K in strikes]
fourier = [s.price for s in hh.solve(hh.BasketPricingProblem(calls, market), hh.CarrMadan(1.0, 100.0, hh.HestonDynamics())).solutions]

n = 1 << 20
seeds = np.arange(1, n + 1)
print(f"{'steps':>5} {'strike':>7} {'Carr-Madan':>11} | {'Euler':>9} {'error':>8} | {'QE':>9} {'error':>8} | {'std error':>9}")
for steps in (8, 16, 32):
    cfg = hh.SimulationConfig(n, steps=steps, seeds=seeds)
    euler = hh.solve(hh.BasketPricingProblem(calls, market), hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg))
    qe = hh.solve(hh.BasketPricingProblem(calls, market), hh.MonteCarlo(hh.HestonDynamics(), hh.HestonQE(), cfg))
    for K, want, e, q in zip(strikes, fourier, euler.solutions, qe.solutions):
        print(f"{steps:5d} {K:7.1f} {want:11.5f} | {e.price:9.5f} {e.price - want:+8.4f} | {q.price:9.5f} {q.price - want:+8.4f} | "
              f"{q.std_error:9.5f}")

steps = 20
quarterly = hh.Monitoring(every=1)
method = hh.MonteCarlo(hh.HestonDynamics(), hh.HestonQE(martingale=True),
                       hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=hh.Antithetic()))
payoffs = {
    "Asian call (arithmetic, quarterly)": hh.AsianOption(100.0, expiry, hh.Call(), hh.ArithmeticAverage(), quarterly),
    "down-and-out call, B = 60": hh.BarrierOption(100.0, 60.0, expiry, hh.Call(), hh.DownAndOut(), monitoring=quarterly),
    "vanilla call": calls[1],
}
print()
basket = hh.solve(hh.BasketPricingProblem(list(payoffs.values()), market), method)
for name, sol in zip(payoffs, basket.solutions):
    print(f"QE, martingale-corrected  {name:36s} {sol.price:9.5f} +- {sol.std_error:.5f}")
r = basket.solutions[0].result
print(f"one call: {r.kernel_ms:.2f} ms on the device for {n} antithetic pairs x {steps} steps")
