#!/usr/bin/env python3
"""An up-and-out call under Black–Scholes dynamics, watched on the simulation's dates and watched continuously, against
the closed form of the continuously monitored contract (Reiner–Rubinstein) — and a floating lookback call against
Goldman–Sosin–Gatto's.  The Euler step on the log state is the exact lognormal transition, so the only error of the
discrete rows is the monitoring itself; the bridge rows sample the maximum and minimum between the dates from their
exact laws (hh_mc_solve_path_ex, HH_EXTREMES_BRIDGE) and cost no extra steps.  Needs an MI355X."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

S0, K, B, r, sigma = 100.0, 100.0, 120.0, 0.05, 0.2
ref = hh.Date(2020, 1, 1)
expiry = hh.add_years(ref, 1)
T = hh.yearfrac(ref, expiry)
market = hh.BlackScholesInputs(ref, r, S0, sigma)
n = 1 << 20


def Phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def up_and_out_call():
    sT, D, lam = sigma * math.sqrt(T), math.exp(-r * T), (r + 0.5 * sigma * sigma) / (sigma * sigma)
    x1, x2 = math.log(S0 / K) / sT + lam * sT, math.log(S0 / B) / sT + lam * sT
    y1, y2 = math.log(B * B / (S0 * K)) / sT + lam * sT, math.log(B / S0) / sT + lam * sT
    h = B / S0
    return (S0 * (Phi(x1) - Phi(x2)) - K * D * (Phi(x1 - sT) - Phi(x2 - sT))
            - S0 * h ** (2 * lam) * (Phi(-y2) - Phi(-y1)) + K * D * h ** (2 * lam - 2) * (Phi(-y2 + sT) - Phi(-y1 + sT)))


def floating_lookback_call():
    sT, D, k = sigma * math.sqrt(T), math.exp(-r * T), sigma * sigma / (2 * r)
    a1 = (r + 0.5 * sigma * sigma) * T / sT
    return S0 * (Phi(a1) - k * Phi(-a1) - D * (1 - k) * Phi(a1 - sT))


exact = {"up-and-out call, B = 120": up_and_out_call(), "floating lookback call": floating_lookback_call()}
print(f"{'':28s} {'steps':>5s}  {'on the dates':>22s}  {'continuous (bridge)':>22s}  closed form")
for steps in (16, 252):
    cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1))
    mc = hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg)
    rows = {}
    for label, mon in (("dates", hh.Monitoring(1, True)), ("bridge", hh.ContinuousMonitoring())):
        payoffs = [hh.BarrierOption(K, B, expiry, hh.Call(), hh.UpAndOut(), monitoring=mon),
                   hh.LookbackOption(expiry, hh.Call(), monitoring=mon)]
        rows[label] = hh.solve(hh.BasketPricingProblem(payoffs, market), mc).solutions
    for k, name in enumerate(exact):
        d, b = rows["dates"][k], rows["bridge"][k]
        print(f"{name:28s} {steps:5d}  {d.price:9.4f} ({(d.price - exact[name]) / d.std_error:+6.1f} s.e.)  "
              f"{b.price:9.4f} ({(b.price - exact[name]) / b.std_error:+6.1f} s.e.)  {exact[name]:9.4f}")
