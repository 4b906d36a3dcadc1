#!/usr/bin/env python3
"""An American put under Heston with a violent variance process (κ = 0.5, θ = V0 = 0.16, σ = 1.5, ρ = 0, two years), priced by
Longstaff–Schwartz twice on the same trajectories: regressed on the spot alone, and on the spot AND the variance
(regressors="spot_variance": hh_lsm_solve_path_states, the walk's (log S, V) rows and the induction in two variables) —
beside the European price.  The spot alone does not carry the continuation value here: its policy gives up what the
variance knows.  Euler–Maruyama and the quadratic-exponential scheme side by side.  Needs an MI355X.

    python examples/american_heston_sv.py [trajectories]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

REF = hh.Date(2025, 1, 1)
EXPIRY = hh.add_years(REF, 2)
STEPS, EVERY, DEGREE, STRIKE = 48, 4, 3, 100.0   # 12 exercise dates


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    mkt = hh.HestonInputs(REF, 0.05, 100.0, 0.16, 0.5, 0.16, 1.5, 0.0)
    cfg = hh.SimulationConfig(n, steps=STEPS, seeds=np.arange(1, n + 1, dtype=np.uint64))
    american = hh.PricingProblem(hh.VanillaOption(STRIKE, EXPIRY, hh.American(), hh.Put(), hh.Spot()), mkt)
    european = hh.PricingProblem(hh.VanillaOption(STRIKE, EXPIRY, hh.European(), hh.Put(), hh.Spot()), mkt)
    for name, strategy, kw in (("EulerMaruyama", hh.EulerMaruyama(), dict(path_state="spot")), ("HestonQE", hh.HestonQE(), {})):
        mc = hh.MonteCarlo(hh.HestonDynamics(), strategy, cfg)
        lsm = hh.LSM(mc, DEGREE)
        on_s = hh.solve(american, lsm, exercise_every=EVERY, **kw)
        on_sv = hh.solve(american, lsm, exercise_every=EVERY, regressors="spot_variance", **kw)
        eu = hh.solve(european, mc)
        print(f"{name:14s} LSM on S {on_s.price:8.4f} +- {on_s.std_error:.4f}   LSM on (S, V) {on_sv.price:8.4f} +- {on_sv.std_error:.4f}"
              f"   European {eu.price:8.4f} +- {eu.std_error:.4f}")
        paths = hh.simulate_state_paths(american, mc, exercise_every=EVERY)
        print(f"{'':14s} variance at expiry: mean {paths.variance[-1].mean():.4f}, {100 * np.mean(paths.variance[-1] < 0.01):.1f} % of the "
              f"trajectories below 0.01")
    print(f"{n} trajectories x {STEPS} steps, {STEPS // EVERY} exercise dates, degree {DEGREE}: "
          f"{hh.multiasset.basis_count(2, DEGREE)} basis functions in (S, V)")


if __name__ == "__main__":
    main()
