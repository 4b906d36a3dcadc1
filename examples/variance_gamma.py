#!/usr/bin/env python3
"""Variance Gamma (Madan, Carr and Chang 1998): a vanilla smile by Carr–Madan (every strike's Fourier integral in one
launch, hh_carr_madan_vg) against the gamma-mixing integral and the lognormal model at the matched total variance
σ² + θ²ν, the same prices by Monte Carlo on the terminal law (hh_mc_solve_vg), and an arithmetic Asian call on 12 dates
from one simulation of gamma time-changed paths (hh_mc_solve_path_vg) — exact in law on those dates: no finer grid is
needed.  Needs an MI355X."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2021, 1, 1)
expiry = hh.add_years(ref, 1)
sigma, theta, nu = 0.2, -0.3, 0.5  # θ < 0: a left skew; ν: kurtosis, also at short expiries
market = hh.VarianceGammaInputs(ref, 0.03, 100.0, sigma, theta, nu)
matched = hh.BlackScholesInputs(ref, 0.03, 100.0, math.sqrt(sigma * sigma + theta * theta * nu))
strikes = [70.0, 80.0, 90.0, 100.0, 110.0, 120.0, 130.0]
calls = [hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()) for K in strikes]


def implied_vol(price, K):
    """bisection on the Black–Scholes call"""
    lo, hi = 1e-4, 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        bs = hh.solve(hh.PricingProblem(hh.VanillaOption(K, expiry, hh.European(), hh.Call(), hh.Spot()),
                                        hh.BlackScholesInputs(ref, 0.03, 100.0, mid)), hh.BlackScholesAnalytic()).price
        lo, hi = (mid, hi) if bs < price else (lo, mid)
    return 0.5 * (lo + hi)


# T/ν = 2: the integrand decays like v⁻⁵, so a wide bound
fourier = hh.solve(hh.BasketPricingProblem(calls, market), hh.CarrMadan(1.5, 2000.0, hh.VarianceGammaDynamics()))
n = 1_000_000
config = hh.SimulationConfig(n, steps=12, seeds=np.arange(1, n + 1), variance_reduction=hh.Antithetic())
method = hh.MonteCarlo(hh.VarianceGammaDynamics(), hh.VarianceGammaExact(), config)
print(f"{'strike':>7} {'mixing':>10} {'Carr-Madan':>11} {'difference':>11} {'Monte Carlo':>12} {'+-':>8} {'implied vol':>12} {'lognormal':>10}")
for K, call, cm in zip(strikes, calls, fourier.solutions):
    exact = hh.solve(hh.PricingProblem(call, market), hh.VarianceGammaAnalytic()).price
    mc = hh.solve(hh.PricingProblem(call, market), method)  # one European vanilla: the terminal law
    flat = hh.solve(hh.PricingProblem(call, matched), hh.BlackScholesAnalytic()).price
    print(f"{K:7.1f} {exact:10.6f} {cm.price:11.6f} {cm.price - exact:+11.1e} {mc.price:12.6f} {mc.std_error:8.5f} "
          f"{implied_vol(exact, K):12.4f} {flat:10.6f}")

monthly = hh.Monitoring(every=1)  # 12 steps, 12 dates
payoffs = {
    "Asian call (arithmetic, 12 dates)": hh.AsianOption(100.0, expiry, hh.Call(), hh.ArithmeticAverage(), monthly),
    "down-and-out call, B = 80": hh.BarrierOption(100.0, 80.0, expiry, hh.Call(), hh.DownAndOut(), monitoring=monthly),
    "vanilla call": calls[3],
}
print()
basket = hh.solve(hh.BasketPricingProblem(list(payoffs.values()), market), method)
for name, sol in zip(payoffs, basket.solutions):
    print(f"{name:36s} {sol.price:9.5f} +- {sol.std_error:.5f}")
r = basket.solutions[0].result
print(f"one call: {r.kernel_ms:.2f} ms on the device for {n} antithetic pairs x 12 gamma variates each")
