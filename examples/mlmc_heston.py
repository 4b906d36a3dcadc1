#!/usr/bin/env python3
"""Multilevel Monte Carlo by tolerance: a Heston call (S0 = K = 100, r = 0.03, T = 1, v0 = θ = 0.04, κ = 1.5, σ = 0.3, ρ = −0.7
— the Feller condition holds, the Euler scheme converges strongly and the coupling pays) on Euler–Maruyama levels of 4, 8,
16, … steps, printed level by level, next to a single-level solve on the finest level's steps with the trajectories that
give the same standard error, and to Carr–Madan.  Needs an MI355X."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2021, 1, 1)
expiry = hh.Date(2022, 1, 1)
call = hh.VanillaOption(100.0, expiry, hh.European(), hh.Call(), hh.Spot())
heston = hh.PricingProblem(call, hh.HestonInputs(ref, 0.03, 100.0, 0.04, 1.5, 0.04, 0.3, -0.7))
eps = 0.02

sol = hh.solve(heston, hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.MLMCConfig(4, tolerance=eps, seed=2026)))
print(f"{'level':>5} {'steps':>6} {'trajectories':>12} {'mean':>10} {'variance':>10} {'E[P_l]':>10}")
for l, lv in enumerate(sol.levels):
    print(f"{l:5d} {lv.steps:6d} {lv.trajectories:12d} {lv.mean:10.5f} {lv.variance:10.4f} {lv.fine_mean:10.5f}")
print(f"multilevel   {sol.price:.5f} +- {sol.std_error:.5f}  (tolerance {eps}, converged: {sol.converged}, bias estimate "
      f"{sol.bias_estimate:.4f}, cost {sol.cost:.3g} steps)")

finest = sol.levels[-1].steps
pilot = hh.solve(heston, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                                       hh.SimulationConfig(2 ** 16, steps=finest, seeds=np.arange(1, 2 ** 16 + 1))), ensemble=False)
n = int(math.ceil(2 ** 16 * (pilot.std_error / sol.std_error) ** 2))  # the trajectories of the same standard error
mc = hh.solve(heston, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                                    hh.SimulationConfig(n, steps=finest, seeds=np.arange(1, n + 1))), ensemble=False)
print(f"single level {mc.price:.5f} +- {mc.std_error:.5f}  ({n} trajectories on {finest} steps: cost {n * finest:.3g} steps, "
      f"{n * finest / sol.cost:.1f} times the multilevel solve's)")
print(f"Carr-Madan   {hh.solve(heston, hh.CarrMadan(1.0, 32.0, hh.HestonDynamics())).price:.5f}")
