#!/usr/bin/env python3
"""Path-dependent payoffs on Heston Euler paths in ONE call: an arithmetic Asian call, an up-and-out / up-and-in
barrier pair, a cash-or-nothing digital and the vanilla call they relate to — one simulation of the trajectories, every
payoff evaluated on its running statistics (hh_mc_solve_path).  Needs an MI355X."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
expiry = hh.add_years(ref, 1)
market = hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
n, steps = 500_000, 252
monthly = hh.Monitoring(every=21)  # 12 monitoring dates, the last one the expiry
payoffs = {
    "Asian call (arithmetic, monthly)": hh.AsianOption(100.0, expiry, hh.Call(), hh.ArithmeticAverage(), monthly),
    "up-and-out call, B = 125": hh.BarrierOption(100.0, 125.0, expiry, hh.Call(), hh.UpAndOut(), monitoring=monthly),
    "up-and-in call,  B = 125": hh.BarrierOption(100.0, 125.0, expiry, hh.Call(), hh.UpAndIn(), monitoring=monthly),
    "digital call, pays 10": hh.DigitalOption(100.0, expiry, hh.Call(), hh.CashOrNothing(10.0)),
    "vanilla call": hh.VanillaOption(100.0, expiry, hh.European(), hh.Call(), hh.Spot()),
}
cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1), variance_reduction=hh.Antithetic())
mc = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)
basket = hh.solve(hh.BasketPricingProblem(list(payoffs.values()), market), mc)
for name, sol in zip(payoffs, basket.solutions):
    print(f"{name:34s} {sol.price:9.5f} +- {sol.std_error:.5f}")
r = basket.solutions[0].result
print(f"one call: {r.kernel_ms:.2f} ms on the device for {n} antithetic pairs x {steps} steps, {len(payoffs)} payoffs")
out_, in_, van = (basket.solutions[k].price for k in (1, 2, 4))
print(f"knock-out + knock-in - vanilla = {out_ + in_ - van:+.2e}")
