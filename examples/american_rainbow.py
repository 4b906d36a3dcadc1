#!/usr/bin/env python3
"""American and Bermudan options on two correlated assets by Longstaff–Schwartz with a regression basis in both spots
(hh_lsm_solve_assets: the assets' state rows, then the several-variable induction): a worst-of put and an equal-weight
basket put, each beside its European price and its Bermudan price on four dates, the worst-of put's delta to the first
asset, and the assets' paths on the exercise dates.  Needs an MI355X.

    python examples/american_rainbow.py [trajectories]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

REF = hh.Date(2025, 1, 1)
EXPIRY = hh.add_years(REF, 1)
STEPS, DEGREE, STRIKE = 16, 3, 100.0


def market():
    return hh.MultiAssetInputs(REF, 0.05, spots=(100.0, 100.0), sigmas=(0.2, 0.3), correlation=[[1.0, 0.3], [0.3, 1.0]])


def put(index, style):
    return hh.IndexOption(index, hh.VanillaOption(STRIKE, EXPIRY, style, hh.Put(), hh.Spot()))


def monte_carlo(n):
    cfg = hh.SimulationConfig(n, steps=STEPS, seeds=np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    return hh.MonteCarlo(hh.MultiAssetDynamics(), hh.EulerMaruyama(), cfg)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 17
    mkt, mc = market(), monte_carlo(n)
    lsm = hh.LSM(mc, DEGREE)
    for name, index in (("worst-of put", hh.WorstOf()), ("basket put (1/2, 1/2)", hh.WeightedSum((0.5, 0.5)))):
        american = hh.solve(hh.PricingProblem(put(index, hh.American()), mkt), lsm)
        bermudan = hh.solve(hh.PricingProblem(put(index, hh.American()), mkt), lsm, exercise_every=4)
        european = hh.solve(hh.PricingProblem(put(index, hh.European()), mkt), mc)
        print(f"{name:24s} American {american.price:8.4f} +- {american.std_error:.4f}   Bermudan (4 dates) {bermudan.price:8.4f}"
              f"   European {european.price:8.4f}")
        early = np.mean(american.stopping_info[0] < STEPS)
        print(f"{'':24s} exercised before expiry on {100 * early:.1f} % of the trajectories")
    prob = hh.PricingProblem(put(hh.WorstOf(), hh.American()), mkt)
    delta = hh.solve(hh.GreekProblem(prob, hh.AssetSpotLens(0)), hh.FiniteDifference(1e-2), lsm).greek
    print(f"{'worst-of put':24s} delta to the first asset {delta:8.4f}   (central difference, shared seeds)")
    paths = hh.simulate_asset_paths(prob, mc, exercise_every=4)
    print(f"paths: {paths.spot.shape[0]} dates x {paths.spot.shape[1]} assets x {paths.spot.shape[2]} columns; mean spots at expiry "
          f"{paths.spot[-1].mean(axis=1).round(3)} (forward {100 * np.exp(0.05):.3f})")
    print(f"{n} trajectories x {STEPS} steps, degree {DEGREE}: {hh.multiasset.basis_count(2, DEGREE)} basis functions")


if __name__ == "__main__":
    main()
