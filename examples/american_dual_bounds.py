#!/usr/bin/env python3
"""The American put of american_heston_sv.py (κ = 0.5, θ = V0 = 0.16, σ = 1.5, ρ = 0, two years, 12 exercise dates) with a
BRACKET instead of one in-sample number: the LSM policy on (S, V) is fitted on one set of trajectories, valued on fresh ones —
a true lower bound, free of look-ahead bias — and bounded from above by the Andersen–Broadie dual: a martingale built from
nested simulation under that policy (hh_lsm_upper_bound).  The regression on S alone cannot be bracketed this way by the
library (its induction keeps no policy); the bracket says how good the regression on (S, V) is.  Needs an MI355X.

    python examples/american_dual_bounds.py [trajectories] [outer] [inner]
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
    outer = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    inner = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    mkt = hh.HestonInputs(REF, 0.05, 100.0, 0.16, 0.5, 0.16, 1.5, 0.0)
    cfg = hh.SimulationConfig(n, steps=STEPS, seeds=np.arange(1, n + 1, dtype=np.uint64))
    american = hh.PricingProblem(hh.VanillaOption(STRIKE, EXPIRY, hh.American(), hh.Put(), hh.Spot()), mkt)
    lsm = hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, DEGREE)
    # fresh: as many seeds again, after the fit's; outer: the next `outer` seeds
    sol = hh.solve(american, hh.DualBounds(lsm, outer=outer, inner=inner, fresh=n, inner_seed=2024), exercise_every=EVERY)
    print(f"in sample (neither bound)  {sol.in_sample:8.4f} +- {sol.in_sample_se:.4f}")
    print(f"lower: policy on fresh     {sol.lower:8.4f} +- {sol.lower_se:.4f}")
    print(f"upper: dual, nested        {sol.upper:8.4f} +- {sol.upper_se:.4f}")
    print(f"gap                        {sol.gap:8.4f} +- {sol.gap_se:.4f}")
    # the same bound under the policy that never exercises early: what an uninformative martingale gives
    never = np.zeros_like(sol.policy.array)
    never[:, 2:4], never[:, 4] = 1.0, 1e300
    hand = hh.ExercisePolicy(never, 2, DEGREE, STEPS // EVERY, sol.policy.discount, EVERY)
    res = hh.upper_bound(american, lsm, hand, np.arange(2 * n + 1, 2 * n + 1 + outer, dtype=np.uint64), inner=inner, inner_seed=2024)
    print(f"upper, never-exercise      {res.upper:8.4f} +- {res.upper_se:.4f}")
    print(f"{n} fitted and {n} fresh trajectories x {STEPS} steps, {STEPS // EVERY} dates, degree {DEGREE}; {outer} outer x {inner} inner "
          f"walks: nested kernel {sol.result.nested_ms:.2f} ms, outer kernel {sol.result.outer_ms:.3f} ms")


if __name__ == "__main__":
    main()
