#!/usr/bin/env python3
"""A European and an American put on the forward by the Cox–Ross–Rubinstein tree on the device, beside the
Black–Scholes price of the European one — the comparison of the reference's examples/black_vs_binomial_tree.jl.
Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hedgehog_jl_amd as hh  # noqa: E402

ref = hh.Date(2020, 1, 1)
expiry = hh.Date(2021, 1, 1)
market = hh.BlackScholesInputs(ref, 0.2, 1.0, 0.4)
euro = hh.VanillaOption(1.2, expiry, hh.European(), hh.Put(), hh.Forward())
american = hh.VanillaOption(1.2, expiry, hh.American(), hh.Put(), hh.Forward())

crr = hh.CoxRossRubinsteinMethod(800)
print("Cox-Ross-Rubinstein European price:", hh.solve(hh.PricingProblem(euro, market), crr).price)
print("Cox-Ross-Rubinstein American price:", hh.solve(hh.PricingProblem(american, market), crr).price)
print("Black-Scholes European price:      ", hh.solve(hh.PricingProblem(euro, market), hh.BlackScholesAnalytic()).price)
