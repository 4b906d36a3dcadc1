#!/usr/bin/env python3
"""Stochastic volatility with jumps on one market (κ = 2, θ = v₀ = 0.04, σ = 0.5, ρ = −0.7, r = 3 %; jumps λ = 0.8,
μ_J = −0.1, σ_J = 0.15): Carr–Madan calls across strikes at three months and at one year, for Heston alone and for
Bates — the jumps steepen the short-dated skew, which the variance process alone cannot —, quadratic-exponential Monte
Carlo prices with their standard errors beside the Bates row (one simulation per expiry, hh_mc_solve_path_bates), and a
monthly monitored down-and-out call, for which no Fourier price exists.  Needs an MI355X."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
heston = hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.5, -0.7)
bates = hh.BatesInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.5, -0.7, 0.8, -0.1, 0.15)
strikes = [80.0, 90.0, 100.0, 110.0, 120.0]
n = 1 << 18
seeds = np.arange(1, n + 1)

for label, expiry, steps in (("three months", hh.Date(2020, 4, 1), 12), ("one year", hh.Date(2021, 1, 1), 48)):
    calls = [hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()) for K in strikes]
    h = hh.solve(hh.BasketPricingProblem(calls, heston), hh.CarrMadan(1.0, 200.0, hh.HestonDynamics())).solutions
    b = hh.solve(hh.BasketPricingProblem(calls, bates), hh.CarrMadan(1.0, 200.0, hh.BatesDynamics())).solutions
    method = hh.MonteCarlo(hh.BatesDynamics(), hh.HestonQE(martingale=True),
                           hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=hh.Antithetic()))
    mc = hh.solve(hh.BasketPricingProblem(calls, bates), method).solutions
    print(f"\n{label}: {'strike':>7} | {'Heston':>9} | {'Bates':>9} | {'Bates, QE Monte Carlo':>24}")
    for K, sh, sb, sm in zip(strikes, h, b, mc):
        print(f"{'':{len(label) + 1}} {K:7.1f} | {sh.price:9.5f} | {sb.price:9.5f} | {sm.price:9.5f} +- {sm.std_error:.5f} "
              f"({(sm.price - sb.price) / sm.std_error:+.2f})")

expiry, steps = hh.Date(2021, 1, 1), 48
monthly = hh.Monitoring(every=4)
method = hh.MonteCarlo(hh.BatesDynamics(), hh.HestonQE(martingale=True),
                       hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=hh.Antithetic()))
barrier = hh.BarrierOption(100.0, 80.0, expiry, hh.Call(), hh.DownAndOut(), monitoring=monthly)
sol = hh.solve(hh.PricingProblem(barrier, bates), method)
print(f"\ndown-and-out call, K = 100, B = 80, monitored monthly, one year (Bates): {sol.price:.5f} +- {sol.std_error:.5f}")
print(f"one call: {sol.result.kernel_ms:.2f} ms on the device for {n} antithetic pairs x {steps} steps")
