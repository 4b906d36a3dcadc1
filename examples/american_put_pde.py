#!/usr/bin/env python3
"""An American put on a Crank–Nicolson grid on the device, with the delta and gamma the grid gives for free, beside
the Cox–Ross–Rubinstein tree and a bumped-spot delta through the same solver; then a strike ladder in one launch.
Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
expiry = hh.Date(2021, 1, 1)
market = hh.BlackScholesInputs(ref, 0.05, 100.0, 0.2)
put = hh.VanillaOption(100.0, expiry, hh.American(), hh.Put(), hh.Spot())
prob = hh.PricingProblem(put, market)

grid = hh.CrankNicolsonMethod(512, 256)   # 512 intervals in log-spot, 256 time steps, the first 2 as Rannacher steps
sol = hh.solve(prob, grid)
print(f"Crank-Nicolson (512, 256): price {sol.price:.6f}  delta {sol.delta:.6f}  gamma {sol.gamma:.6f}")
print(f"Cox-Ross-Rubinstein 2000:  price {hh.solve(prob, hh.CoxRossRubinsteinMethod(2000)).price:.6f}")
bumped = hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.FiniteDifference(1e-2, hh.FDCentral()), grid).greek
print(f"bumped-spot delta through the grid: {bumped:.6f}")

strikes = [80.0 + 5.0 * k for k in range(9)]
ladder = hh.solve(hh.BasketPricingProblem([hh.VanillaOption(K, expiry, hh.American(), hh.Put(), hh.Spot())
                                           for K in strikes], market), grid)
for K, s in zip(strikes, ladder.solutions):
    print(f"K = {K:6.1f}: price {s.price:9.6f}  delta {s.delta:9.6f}  gamma {s.gamma:.6f}")
