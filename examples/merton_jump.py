#!/usr/bin/env python3
"""Merton (1976) jump diffusion: a vanilla smile by Carr–Madan (every strike's Fourier integral in one launch,
hh_carr_madan_jump) against Merton's series, the same prices by Monte Carlo on the terminal law (hh_mc_solve_jump), and
an arithmetic Asian and a down-and-out call under jumps from one simulation of Euler paths (hh_mc_solve_path_jump).
Needs an MI355X."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
expiry = hh.add_years(ref, 1)
# 0.8 jumps a year, 10 % down on average with a spread of 15 %: a left skew the lognormal model cannot make
market = hh.MertonInputs(ref, 0.03, 100.0, 0.2, 0.8, -0.1, 0.15)
flat = market.black_scholes()
strikes = [70.0, 80.0, 90.0, 100.0, 110.0, 120.0, 130.0]
calls = [hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()) for K in strikes]


def implied_vol(price, K):
    """bisection on the Black–Scholes call"""
    lo, hi = 1e-4, 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        bs = hh.solve(hh.PricingProblem(hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()),
                                        hh.BlackScholesInputs(ref, flat.rate, 100.0, mid)), hh.BlackScholesAnalytic()).price
        lo, hi = (mid, hi) if bs < price else (lo, mid)
    return 0.5 * (lo + hi)


fourier = hh.solve(hh.BasketPricingProblem(calls, market), hh.CarrMadan(1.0, 200.0, hh.MertonDynamics()))
n = 1_000_000
exact = hh.MonteCarlo(hh.MertonDynamics(), hh.MertonExact(),
                      hh.SimulationConfig(n, seeds=np.arange(1, n + 1), variance_reduction=hh.Antithetic()))
sampled = hh.solve(hh.BasketPricingProblem(calls, market), exact)
print(f"{'strike':>7} {'series':>10} {'Carr-Madan':>11} {'difference':>11} {'Monte Carlo':>12} {'+-':>8} {'implied vol':>12}")
for K, call, cm, mc in zip(strikes, calls, fourier.solutions, sampled.solutions):
    series = hh.solve(hh.PricingProblem(call, market), hh.MertonAnalytic()).price
    print(f"{K:7.1f} {series:10.6f} {cm.price:11.6f} {cm.price - series:+11.1e} {mc.price:12.6f} {mc.std_error:8.5f} "
          f"{implied_vol(series, K):12.4f}")

steps = 252
paths = hh.MonteCarlo(hh.MertonDynamics(), hh.EulerMaruyama(),
                      hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1), variance_reduction=hh.Antithetic()))
monthly = hh.Monitoring(every=21)
payoffs = {
    "Asian call (arithmetic, monthly)": hh.AsianOption(100.0, expiry, hh.Call(), hh.ArithmeticAverage(), monthly),
    "down-and-out call, B = 80": hh.BarrierOption(100.0, 80.0, expiry, hh.Call(), hh.DownAndOut(), monitoring=monthly),
    "vanilla call": calls[3],
}
print()
for label, mkt, method in (("with jumps", market, paths),
                           ("without", flat, hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), paths.config))):
    basket = hh.solve(hh.BasketPricingProblem(list(payoffs.values()), mkt), method)
    for name, sol in zip(payoffs, basket.solutions):
        print(f"{label:11s} {name:34s} {sol.price:9.5f} +- {sol.std_error:.5f}")
    r = basket.solutions[0].result
    print(f"{label:11s} one call: {r.kernel_ms:.2f} ms on the device for {n} antithetic pairs x {steps} steps")
print(f"(compensated drift: the discounted spot stays a martingale, E S_T = {100.0 * math.exp(0.03 * hh.yearfrac(ref, expiry)):.4f})")
