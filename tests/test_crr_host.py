"""Host side of the Cox–Ross–Rubinstein trees (no GPU): the per-tree scalars against the reference's formulas
(cox_ross_rubinstein.jl:107-132, :75-81), one spot-factor row per expiry, dispatch through `solve` and
`solve_basket`, and the refusals — bad step counts, Heston inputs, Dual inputs."""
import math

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi, trees
from hedgehog_jl_amd.dates import MILLISECONDS_IN_YEAR_365

REF = hh.Date(2020, 1, 1)


def curve():
    return hh.RateCurve(REF, [0.25, 0.5, 1.0, 2.0], [math.exp(-0.01 * 0.25), math.exp(-0.02 * 0.5),
                                                     math.exp(-0.04 * 1.0), math.exp(-0.05 * 2.0)])


@pytest.mark.parametrize("rate", [0.03, "curve"])
def test_host_scalars_are_the_reference_formulas(rate):
    rc = curve() if rate == "curve" else rate
    m = hh.BlackScholesInputs(REF, rc, 100.0, 0.25)
    expiries = [hh.Date(2020, 9, 1), hh.Date(2021, 8, 15)]
    payoffs = [hh.VanillaOption(K, e, ex, hh.Put(), und) for e in expiries for K in (90.0, 110.0)
               for ex, und in ((hh.American(), hh.Spot()), (hh.American(), hh.Forward()), (hh.European(), hh.Spot()))]
    N = 50
    inp = trees.crr_inputs(payoffs, m, N)
    for k, p in enumerate(payoffs):
        T = (p.expiry - m.referenceDate) / MILLISECONDS_IN_YEAR_365
        dT = T / N
        z = rc if rate != "curve" else rc.interpolate((p.expiry - rc.reference_date) / MILLISECONDS_IN_YEAR_365)
        assert inp.forwards[k] == 100.0 / math.exp(-z * T)
        assert inp.ups[k] == math.exp(0.25 * math.sqrt(dT))
        assert inp.discounts[k] == math.exp(-z * dT)
        assert inp.strikes[k] == p.strike and inp.cps[k] == -1.0
        style = {(hh.American(), hh.Spot()): _ffi.HH_CRR_AMERICAN_SPOT,
                 (hh.American(), hh.Forward()): _ffi.HH_CRR_AMERICAN_FORWARD}.get(
            (p.exercise_style, p.underlying), _ffi.HH_CRR_EUROPEAN)
        assert inp.styles[k] == style
        if style == _ffi.HH_CRR_AMERICAN_SPOT:
            row = inp.spot_factors[inp.spot_row_of_tree[k]]
            for i in (0, 1, N // 2, N - 1):
                t_i = REF_TICKS() + (i * dT) * MILLISECONDS_IN_YEAR_365
                z_i = rc if rate != "curve" else rc.interpolate((t_i - rc.reference_date) / MILLISECONDS_IN_YEAR_365)
                assert row[i] == math.exp(-z_i * (N - i) * dT)
    # one row per expiry, shared by that expiry's Spot American payoffs
    assert inp.spot_factors.shape == (2, N)
    spot_am = [k for k in range(len(payoffs)) if inp.styles[k] == _ffi.HH_CRR_AMERICAN_SPOT]
    assert [int(inp.spot_row_of_tree[k]) for k in spot_am] == [0, 0, 1, 1]
    if rate == "curve":  # the rate at tᵢ moves along the curve
        assert len(set(np.round(np.log(inp.spot_factors[1]) / ((N - np.arange(N)) * 1.0), 12))) > 1


def REF_TICKS():
    return hh.to_ticks(REF)


def test_dispatch_through_solve_and_solve_basket(monkeypatch):
    seen = []

    def fake(inp, steps, device=0):
        seen.append((len(inp.forwards), steps, device))
        return np.arange(len(inp.forwards), dtype=np.float64) + 0.5

    monkeypatch.setattr(trees, "crr_device_prices", fake)
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    p1 = hh.VanillaOption(100.0, hh.Date(2021, 1, 1), hh.American(), hh.Put(), hh.Spot())
    p2 = hh.VanillaOption(90.0, hh.Date(2021, 1, 1), hh.European(), hh.Call(), hh.Forward())
    sol = hh.solve(hh.PricingProblem(p1, m), hh.CoxRossRubinsteinMethod(200, device=1))
    assert isinstance(sol, hh.CRRSolution) and sol.price == 0.5 and sol.method.steps == 200
    b = hh.solve(hh.BasketPricingProblem([p1, p2], m), hh.CoxRossRubinsteinMethod(100))
    assert isinstance(b, hh.BasketPricingSolution)
    assert [s.price for s in b.solutions] == [0.5, 1.5]
    assert all(isinstance(s, hh.CRRSolution) for s in b.solutions)
    assert b.solutions[1].problem == hh.PricingProblem(p2, m)
    assert seen == [(1, 200, 1), (2, 100, 0)]


def test_refusals():
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    p = hh.VanillaOption(100.0, hh.Date(2021, 1, 1), hh.American(), hh.Put(), hh.Spot())
    for steps in (0, -3, _ffi.HH_CRR_MAX_STEPS + 1):
        with pytest.raises(ValueError):
            hh.solve(hh.PricingProblem(p, m), hh.CoxRossRubinsteinMethod(steps))
    heston = hh.HestonInputs(REF, 0.05, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(p, heston), hh.CoxRossRubinsteinMethod(100))
    d = hh.Dual(1.0, (1.0,))
    for dual_prob in (hh.PricingProblem(p, hh.BlackScholesInputs(REF, 0.05, 100.0 * d, 0.2)),
                      hh.PricingProblem(p, hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2 * d)),
                      hh.PricingProblem(p, hh.BlackScholesInputs(REF, 0.05 * d, 100.0, 0.2)),
                      hh.PricingProblem(hh.VanillaOption(100.0 * d, hh.Date(2021, 1, 1), hh.American(), hh.Put(),
                                                         hh.Spot()), m)):
        with pytest.raises(hh.MethodError, match="FiniteDifference"):
            hh.solve(dual_prob, hh.CoxRossRubinsteinMethod(100))
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.GreekProblem(hh.PricingProblem(p, m), hh.SpotLens()), hh.ForwardAD(),
                 hh.CoxRossRubinsteinMethod(100))
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.BasketPricingProblem([p, hh.VanillaOption(100.0 * d, hh.Date(2021, 1, 1), hh.European(),
                                                              hh.Call(), hh.Spot())], m),
                 hh.CoxRossRubinsteinMethod(100))
