#!/usr/bin/env python3
"""Local volatility from a Heston surface (κ = 2, θ = v₀ = 0.04, σ = 0.5, ρ = −0.7, r = 3 %): Carr–Madan call prices on
the stencils of a grid → Dupire's formula (dupire_from) → a LocalVolSurface; the one-year vanillas priced back on
local-volatility paths beside the Carr–Madan prices the table was made of; and a continuously monitored up-and-out call
under local volatility beside the same option on Heston Euler paths — two models that agree on every vanilla and
disagree on the barrier.  Needs an MI355X."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref, expiry = hh.Date(2020, 1, 1), hh.Date(2021, 1, 1)
heston = hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.5, -0.7)
cm = hh.CarrMadan(1.0, 200.0, hh.HestonDynamics())
x0 = math.log(100.0)
times = [0.05 * (j + 1) for j in range(21)]
surface = hh.dupire_from(heston, cm, times, x0 - 1.0, x0 + 1.0, 129, dk=0.02, dT=0.01, vol_bounds=(0.03, 1.5))
local = hh.LocalVolInputs(ref, 0.03, 100.0, surface)
print("local volatility at one year, S = 70 / 100 / 130:",
      " / ".join(f"{hh.get_local_vol(surface, 1.0, S):.4f}" for S in (70.0, 100.0, 130.0)))

n, steps = 1 << 18, 128
seeds = np.arange(1, n + 1)
config = hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=hh.Antithetic())
lv = hh.MonteCarlo(hh.LocalVolDynamics(), hh.EulerMaruyama(), config)
strikes = [80.0, 90.0, 100.0, 110.0, 120.0]
calls = [hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()) for K in strikes]
want = hh.solve(hh.BasketPricingProblem(calls, heston), cm).solutions
got = hh.solve(hh.BasketPricingProblem(calls, local), lv).solutions
print(f"\none year: {'strike':>7} | {'Heston, Carr–Madan':>18} | {'local vol, Monte Carlo':>24}")
for K, w, g in zip(strikes, want, got):
    print(f"{'':9} {K:7.1f} | {w.price:18.5f} | {g.price:9.5f} +- {g.std_error:.5f} ({(g.price - w.price) / g.std_error:+.2f})")

barrier = hh.BarrierOption(100.0, 125.0, expiry, hh.Call(), hh.UpAndOut(), monitoring=hh.ContinuousMonitoring())
a = hh.solve(hh.PricingProblem(barrier, local), lv)
b = hh.solve(hh.PricingProblem(barrier, heston), hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), config))
print(f"\nup-and-out call, K = 100, B = 125, continuously monitored (Brownian bridge), one year:")
print(f"  local volatility  {a.price:.5f} +- {a.std_error:.5f}   ({a.result.kernel_ms:.2f} ms on the device)")
print(f"  Heston, Euler     {b.price:.5f} +- {b.std_error:.5f}   ({b.result.kernel_ms:.2f} ms on the device)")
