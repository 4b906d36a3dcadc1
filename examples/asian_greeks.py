#!/usr/bin/env python3
"""Greeks of an arithmetic Asian call and a floating lookback call on Heston Euler paths: delta and the four
Heston sensitivities from ONE simulation pass with Pathwise() (hh_mc_solve_path_tangent), beside the central finite
differences that take two bumped passes per lens on the same seeds.  Needs an MI355X."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
expiry = hh.add_years(ref, 1)
market = hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
n, steps = 200_000, 252
monthly = hh.Monitoring(every=21)
payoffs = {"Asian call (arithmetic, monthly)": hh.AsianOption(100.0, expiry, hh.Call(), hh.ArithmeticAverage(), monthly),
           "floating lookback call (monthly)": hh.LookbackOption(expiry, hh.Call(), None, hh.Monitoring(21, True))}
lenses = {"delta": hh.SpotLens(), "dV0": hh.optic("market_inputs.V0"),
          "dkappa": hh.optic("market_inputs.κ"), "dtheta": hh.optic("market_inputs.θ"), "dsigma": hh.optic("market_inputs.σ")}
cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1), variance_reduction=hh.Antithetic())
mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
for name, payoff in payoffs.items():
    batch = hh.BatchGreekProblem(hh.PricingProblem(payoff, market), tuple(lenses.values()))
    hh.solve(batch, hh.Pathwise(), mc)  # the first call of a size grows the context's buffers
    t0 = time.perf_counter()
    pathwise = hh.solve(batch, hh.Pathwise(), mc)
    t1 = time.perf_counter()
    bumped = hh.solve(batch, hh.FiniteDifference(1e-4), mc)
    t2 = time.perf_counter()
    print(f"{name}: one tangent pass {1e3 * (t1 - t0):.1f} ms, {2 * len(lenses)} bumped passes {1e3 * (t2 - t1):.1f} ms (wall)")
    for label, lens in lenses.items():
        print(f"  {label:7s} pathwise {pathwise[lens]:+11.6f}   central difference {bumped[lens]:+11.6f}")
