#!/usr/bin/env python3
"""American and Bermudan puts where the library has no tree and no grid: least-squares Monte Carlo on the date rows of the
spot-path models' own kernels (hh_lsm_solve_path).  One at-the-money one-year put under Merton jumps, Heston by the
quadratic-exponential scheme, Bates, Variance Gamma and a skewed local-volatility surface: the European price on the same
trajectories, the Bermudan price on 5 exercise dates and the American one on 50 — fine steps for the law of the paths,
far fewer dates for the regression (exercise_every).  Then the dates of one Variance Gamma trajectory and where its
holder stopped.  Needs an MI355X."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref, expiry = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
r, S0, K = 0.03, 100.0, 100.0
x = math.log(S0) - 1.0 + 2.0 / 128 * np.arange(129)
skew = hh.LocalVolSurface([0.25, 0.75], x, np.vstack([0.2 - 0.15 * (x - math.log(S0)), 0.22 - 0.10 * (x - math.log(S0))]).clip(0.05, 0.6))
qe = hh.HestonQE(1.5, True)
models = [
    ("Merton jumps, Euler", hh.MertonInputs(ref, r, S0, 0.2, 0.8, -0.1, 0.15), hh.MertonDynamics(), hh.EulerMaruyama(), 100),
    ("Heston, QE", hh.HestonInputs(ref, r, S0, 0.04, 2.0, 0.04, 0.3, -0.7), hh.HestonDynamics(), qe, 100),
    ("Bates, QE + jumps", hh.BatesInputs(ref, r, S0, 0.04, 2.0, 0.04, 0.3, -0.7, 0.8, -0.1, 0.15), hh.BatesDynamics(), qe, 100),
    ("local volatility", hh.LocalVolInputs(ref, r, S0, skew), hh.LocalVolDynamics(), hh.EulerMaruyama(), 100),
    ("Variance Gamma", hh.VarianceGammaInputs(ref, r, S0, 0.2, -0.3, 0.5), hh.VarianceGammaDynamics(), hh.VarianceGammaExact(), 50),
]
n = 200_000
seeds = np.arange(1, n + 1, dtype=np.uint64)
american = hh.VanillaOption(K, expiry, hh.American(), hh.Put(), hh.Spot())

print(f"put, K = {K:g}, one year, {n} trajectories and their mirrors, degree 3\n")
print(f"{'model':<22}{'steps':>6} | {'one date (European)':>22} | {'5 dates':>20} | {'50 dates':>20} | device ms")
for name, market, dynamics, strategy, steps in models:
    config = hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=hh.Antithetic())
    lsm = hh.LSM(dynamics, strategy, config, 3)
    prob = hh.PricingProblem(american, market)
    cells = []
    for dates in (1, 5, 50):
        sol = hh.solve(prob, lsm, exercise_every=steps // dates, stopping_info=False)
        cells.append(f"{sol.price:9.4f} +- {sol.std_error:.4f}")
    print(f"{name:<22}{steps:>6} | {cells[0]:>22} | {cells[1]:>20} | {cells[2]:>20} | {sol.result.kernel_ms:.2f}")

# the dates themselves: the rows the regression read, and the date each holder stopped on (in exercise dates, not steps)
name, market, dynamics, strategy, steps = models[-1]
small = hh.SimulationConfig(8, steps=steps, seeds=seeds[:8])
sol = hh.solve(hh.PricingProblem(american, market), hh.LSM(dynamics, strategy, hh.SimulationConfig(n, steps=steps, seeds=seeds), 3),
               exercise_every=10, spot_paths=True)
paths = hh.simulate_spot_paths(hh.PricingProblem(american, market), hh.MonteCarlo(dynamics, strategy, small), exercise_every=10)
assert np.array_equal(paths.spot, sol.spot_paths[:, :8])  # the same seeds: the same trajectories
tau, value = sol.stopping_info
print(f"\n{name}, 5 exercise dates at t = " + ", ".join(f"{t:.1f}" for t in paths.times[1:]))
for i in range(4):
    print(f"  trajectory {i}: " + "  ".join(f"{s:7.2f}" for s in paths.spot[:, i]) + f"   stopped on date {tau[i]}, worth {value[i]:.2f} there")
