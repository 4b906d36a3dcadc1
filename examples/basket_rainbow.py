#!/usr/bin/env python3
"""Options on several correlated assets from one call: an arithmetic basket call, its Asian and up-and-out forms, a
spread option and a worst-of put (hh_mc_solve_path_assets: one statistics pass per distinct index, all on the same
seeds), each with its standard error; and the call on the geometric index against its closed form.  Needs an MI355X.

    python examples/basket_rainbow.py [trajectories]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

REF = hh.Date(2025, 1, 1)
EXPIRY = hh.add_years(REF, 1)
WEIGHTS = (0.5, 0.3, 0.2)
STEPS = 12


def market():
    """three assets: the first two move together, the third against the first"""
    return hh.MultiAssetInputs(REF, 0.03, spots=(100.0, 90.0, 110.0), sigmas=(0.2, 0.35, 0.25),
                               correlation=[[1.0, 0.6, -0.3], [0.6, 1.0, 0.2], [-0.3, 0.2, 1.0]])


def options():
    """name -> IndexOption; the first three share the basket index and so one simulation"""
    basket, monthly = hh.WeightedSum(WEIGHTS), hh.Monitoring(every=1)
    call = lambda K, cp=None: hh.VanillaOption(K, EXPIRY, hh.European(), cp or hh.Call(), hh.Spot())  # noqa: E731
    return {
        "basket call, K = 100": hh.IndexOption(basket, call(100.0)),
        "Asian basket call (arithmetic, monthly)": hh.IndexOption(basket, hh.AsianOption(100.0, EXPIRY, hh.Call(), hh.ArithmeticAverage(), monthly)),
        "up-and-out basket call, B = 125": hh.IndexOption(basket, hh.BarrierOption(100.0, 125.0, EXPIRY, hh.Call(), hh.UpAndOut(), monitoring=monthly)),
        "spread call S1 - S2, K = 5": hh.IndexOption(hh.WeightedSum((1.0, -1.0, 0.0)), call(5.0)),
        "worst-of put, K = 95": hh.IndexOption(hh.WorstOf(), call(95.0, hh.Put())),
        "geometric index call, K = 100": hh.IndexOption(hh.GeometricMean(WEIGHTS), call(100.0)),
    }


def method(n, antithetic=True):
    cfg = hh.SimulationConfig(n, steps=STEPS, seeds=np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15),
                              variance_reduction=hh.Antithetic() if antithetic else hh.NoVarianceReduction())
    return hh.MonteCarlo(hh.MultiAssetDynamics(), hh.EulerMaruyama(), cfg)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    opts, mkt = options(), market()
    out = hh.solve(hh.BasketPricingProblem(list(opts.values()), mkt), method(n))
    for name, sol in zip(opts, out.solutions):
        print(f"{name:42s} {sol.price:9.5f} +- {sol.std_error:.5f}")
    geo = list(opts.values())[-1]
    closed = hh.solve(hh.PricingProblem(geo, mkt), hh.MultiAssetAnalytic()).price
    sol = out.solutions[-1]
    print(f"{'  its closed form':42s} {closed:9.5f}   ({(sol.price - closed) / sol.std_error:+.2f} standard errors)")
    delta = hh.solve(hh.GreekProblem(hh.PricingProblem(geo, mkt), hh.AssetSpotLens(0)), hh.FiniteDifference(1e-3), method(n)).greek
    print(f"{'  its delta to the first asset':42s} {delta:9.5f}   (central difference, shared seeds)")
    print(f"{n} antithetic pairs x {STEPS} steps, {len({o.index for o in opts.values()})} statistics passes")


if __name__ == "__main__":
    main()
