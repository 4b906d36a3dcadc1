#!/usr/bin/env python3
"""Randomised quasi-Monte Carlo beside pseudo-random Monte Carlo at equal budget: a Heston call (S0 = K = 100, r = 0.03,
T = 1, v0 = θ = 0.04, κ = 1.5, σ = 0.5, ρ = −0.7) by Euler–Maruyama on 16, 64 and 252 steps — 16 digital shifts of 2^14
Sobol' points with the Brownian-bridge and the incremental construction, against 16·2^14 pseudo-random trajectories on the
same steps — and the one-dimensional exact lognormal law against Black–Scholes.  Needs an MI355X."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2021, 1, 1)
expiry = hh.Date(2022, 1, 1)
call = hh.VanillaOption(100.0, expiry, hh.European(), hh.Call(), hh.Spot())
heston = hh.PricingProblem(call, hh.HestonInputs(ref, 0.03, 100.0, 0.04, 1.5, 0.04, 0.5, -0.7))
n, R, seed = 1 << 14, 16, 2026

print(f"{'steps':>5} | {'bridge':>10} {'std error':>9} | {'incremental':>11} {'std error':>9} | {'pseudo-random':>13} {'std error':>9} | "
      f"{'MC / bridge':>11}")
for steps in (16, 64, 252):
    sols = [hh.solve(heston, hh.QuasiMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                                                hh.SobolConfig(n, steps=steps, randomizations=R, seed=seed, construction=c)))
            for c in (hh.BrownianBridge(), hh.Incremental())]
    mc = hh.solve(heston, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                                        hh.SimulationConfig(R * n, steps=steps, seeds=np.arange(1, R * n + 1))), ensemble=False)
    print(f"{steps:5d} | {sols[0].price:10.5f} {sols[0].std_error:9.5f} | {sols[1].price:11.5f} {sols[1].std_error:9.5f} | "
          f"{mc.price:13.5f} {mc.std_error:9.5f} | {mc.std_error / sols[0].std_error:11.1f}")

black = hh.PricingProblem(call, hh.BlackScholesInputs(ref, 0.03, 100.0, 0.2))
exact = hh.solve(black, hh.BlackScholesAnalytic()).price
q = hh.solve(black, hh.QuasiMonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(), hh.SobolConfig(1 << 12, randomizations=R, seed=seed)))
mc = hh.solve(black, hh.MonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(), hh.SimulationConfig(R << 12, seeds=np.arange(1, (R << 12) + 1))), ensemble=False)
print(f"\nexact lognormal law, Black–Scholes {exact:.6f}: RQMC {q.price:.6f} +- {q.std_error:.6f} ({R} x 2^12 points), "
      f"pseudo-random {mc.price:.6f} +- {mc.std_error:.6f} ({R << 12} trajectories)")
