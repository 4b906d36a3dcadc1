"""Cox–Ross–Rubinstein trees on the device (hh_crr_solve, csrc/hh_crr.hip) through `solve`: the reference's pinned
prices (test/unit/binomial_tree.jl), bit identity with the numpy restatement below, the distance to the numpy oracle
(oracle/analytic.crr_price), a basket equal to single solves, the reference's agreement tests
(price_agreement.jl, american_options.jl) and finite-difference Greeks."""
import math

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from hedgehog_jl_amd.trees import crr_inputs
from oracle import analytic

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
REF = hh.Date(2020, 1, 1)


# ---- the restatement: the fixed node-factor sequence of csrc/hh_crr.hip, then the reference's induction ----
def pw(u: float, e: int) -> float:
    """u^e by left-to-right square-and-multiply; pw(u, 0) = 1."""
    if e == 0:
        return 1.0
    u = float(u)   # a Python float: an overflow to inf is silent, as on the device
    x = u
    for b in range(e.bit_length() - 2, -1, -1):
        x = x * x
        if (e >> b) & 1:
            x = x * u
    return x


def node_factors(u: float, N: int) -> np.ndarray:
    """w[k + N] = u^k for k = −N … N: H·L for k >= 0, (1/H)·(1/L) for k < 0, m = |k|, L = u^(m mod 256),
    H = u^(256·⌊m/256⌋)."""
    L = [pw(u, r) for r in range(256)]
    H = [pw(u, 256 * m) for m in range(N // 256 + 1)]
    w = np.empty(2 * N + 1)
    for k in range(-N, N + 1):
        m = abs(k)
        w[k + N] = H[m >> 8] * L[m & 255] if k >= 0 else (1.0 / H[m >> 8]) * (1.0 / L[m & 255])
    return w


def restated(F, K, cp, u, disc, style, sf_row, N) -> float:
    p = 1.0 / (1.0 + u)
    q = 1.0 - p
    w = node_factors(u, N)
    v = np.maximum(cp * (F * w[np.arange(-N, N + 1, 2) + N] - K), 0.0)
    for i in range(N - 1, -1, -1):
        v = disc * (p * v[1:] + q * v[:-1])
        if style != _ffi.HH_CRR_EUROPEAN:
            S = F * w[np.arange(-i, i + 1, 2) + N]
            if style == _ffi.HH_CRR_AMERICAN_SPOT:
                S = sf_row[i] * S
            v = np.maximum(v, np.maximum(cp * (S - K), 0.0))
    return float(v[0])


def restated_prices(payoffs, m, N):
    inp = crr_inputs(payoffs, m, N)
    return [restated(inp.forwards[k], inp.strikes[k], inp.cps[k], inp.ups[k], inp.discounts[k], inp.styles[k],
                     inp.spot_factors[inp.spot_row_of_tree[k]] if inp.styles[k] == _ffi.HH_CRR_AMERICAN_SPOT else None,
                     N) for k in range(len(payoffs))]


def opt(K, expiry, ex, cp, und):
    return hh.VanillaOption(K, expiry, ex, cp, und)


ALL8 = [(ex, cp, und) for ex in (hh.European(), hh.American()) for cp in (hh.Call(), hh.Put())
        for und in (hh.Spot(), hh.Forward())]


def test_reference_regression_values():
    """binomial_tree.jl:18,26 (atol 1e-8)."""
    m = hh.BlackScholesInputs(REF, 0.2, 1.0, 0.4)
    expiry = REF + __import__("datetime").timedelta(days=365)
    call = hh.solve(hh.PricingProblem(opt(1.0, expiry, hh.American(), hh.Call(), hh.Spot()), m),
                    hh.CoxRossRubinsteinMethod(80))
    put = hh.solve(hh.PricingProblem(opt(1.0, expiry, hh.American(), hh.Put(), hh.Forward()), m),
                   hh.CoxRossRubinsteinMethod(80))
    assert isinstance(call, hh.CRRSolution)
    print(f"\nAmerican call on spot {call.price!r}, American put on forward {put.price!r}")
    assert call.price == pytest.approx(0.25225758542934945, abs=1e-8)
    assert put.price == pytest.approx(0.07409148128021317, abs=1e-8)


FORM_A = _ffi.HH_CRR_FORM_A_MAX_STEPS


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, FORM_A, FORM_A + 1])
def test_bit_identity_with_the_restatement(N):
    """Every style × call/put × Spot/Forward, at and off the money, in one basket call: == the restatement."""
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.3)
    payoffs = [opt(K, hh.Date(2021, 6, 30), ex, cp, und) for ex, cp, und in ALL8 for K in (80.0, 100.0, 130.0)]
    got = hh.solve(hh.BasketPricingProblem(payoffs, m), hh.CoxRossRubinsteinMethod(N))
    want = restated_prices(payoffs, m, N)
    assert [s.price for s in got.solutions] == want


@pytest.mark.parametrize("N", [4096, 32768])
def test_bit_identity_in_form_b(N):
    m = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.25)
    payoffs = [opt(105.0, hh.Date(2021, 1, 1), hh.American(), hh.Put(), hh.Spot()),
               opt(95.0, hh.Date(2020, 7, 1), hh.European(), hh.Call(), hh.Forward())]
    got = [s.price for s in hh.solve(hh.BasketPricingProblem(payoffs, m), hh.CoxRossRubinsteinMethod(N)).solutions]
    assert got == restated_prices(payoffs, m, N)


@pytest.mark.parametrize("sigma,expiry,K", [(0.3, REF, 100.0), (1e-8, hh.Date(2021, 1, 1), 100.0),
                                            (2.0, hh.Date(2022, 1, 1), 100.0), (0.2, hh.Date(2021, 1, 1), 1.0),
                                            (0.2, hh.Date(2021, 1, 1), 1e4)])
def test_bit_identity_at_the_edges(sigma, expiry, K):
    """T = 0, σ = 1e-8, σ = 2, deep in and out of the money."""
    m = hh.BlackScholesInputs(REF, 0.04, 100.0, sigma)
    payoffs = [opt(K, expiry, ex, cp, und) for ex, cp, und in ALL8]
    for N in (1, 65, 700):
        got = [s.price for s in hh.solve(hh.BasketPricingProblem(payoffs, m), hh.CoxRossRubinsteinMethod(N)).solutions]
        assert got == restated_prices(payoffs, m, N)
        assert all(math.isfinite(x) for x in got)


def test_spot_american_on_an_interpolated_curve():
    """Per-step zero rates read off a RateCurve at tᵢ (cox_ross_rubinstein.jl:75-81): == the restatement, and not
    the flat-curve price."""
    curve = hh.RateCurve(REF, [0.25, 0.5, 1.0, 2.0], [math.exp(-0.01 * 0.25), math.exp(-0.02 * 0.5),
                                                      math.exp(-0.04 * 1.0), math.exp(-0.05 * 2.0)])
    m = hh.BlackScholesInputs(REF, curve, 100.0, 0.25)
    payoffs = [opt(K, e, hh.American(), cp, hh.Spot()) for K in (90.0, 110.0) for cp in (hh.Call(), hh.Put())
               for e in (hh.Date(2020, 9, 1), hh.Date(2021, 8, 15))]
    for N in (100, 1000):
        got = [s.price for s in hh.solve(hh.BasketPricingProblem(payoffs, m), hh.CoxRossRubinsteinMethod(N)).solutions]
        assert got == restated_prices(payoffs, m, N)
    inp = crr_inputs(payoffs, m, 100)
    assert inp.spot_factors.shape == (2, 100)   # one row per expiry
    flat = hh.BlackScholesInputs(REF, 0.04, 100.0, 0.25)
    assert hh.solve(hh.PricingProblem(payoffs[2], m), hh.CoxRossRubinsteinMethod(100)).price != \
        hh.solve(hh.PricingProblem(payoffs[2], flat), hh.CoxRossRubinsteinMethod(100)).price


def test_against_the_numpy_oracle():
    """oracle/analytic.crr_price forms u^k with numpy's pow; everything else is the same sequence of operations.
    Bound: the node factors differ by δ_w (measured below: ours against u**k, relative); a leaf or an exercise
    value moves by at most δ_w·S, and the induction (positive weights p, q summing to 1, disc <= 1 for r >= 0,
    max and payoff 1-Lipschitz) carries a node's error to the root with its probability weight, so the price
    moves by at most δ_w·G, G = F·max(1, g^N) >= E[S_i], g = p·u + q/u the one-step mean of the factor.  The
    two inductions also round different numbers: at most 4 roundings per node-step (continuation) plus 3
    (exercise), each <= ε·(G + K) in absolute terms, carried non-expansively over N steps: 7·N·ε·(G + K)."""
    worst = 0.0
    for S0, K, r, sigma, days, N, cp, am, fwd in [
            (100, 100, 0.05, 0.2, 366, 1000, -1.0, True, False), (100, 90, 0.02, 0.4, 730, 2000, -1.0, True, False),
            (120, 100, 0.15, 0.3, 366, 800, 1.0, True, False), (100, 110, 0.0, 0.1, 182, 500, 1.0, False, False),
            (1.0, 1.0, 0.2, 0.4, 365, 80, -1.0, True, True), (100, 80, 0.05, 0.25, 547, 1500, -1.0, True, True)]:
        expiry = REF + __import__("datetime").timedelta(days=days)
        T = hh.yearfrac(REF, expiry)
        payoff = opt(float(K), expiry, hh.American() if am else hh.European(), hh.Call() if cp > 0 else hh.Put(),
                     hh.Forward() if fwd else hh.Spot())
        got = hh.solve(hh.PricingProblem(payoff, hh.BlackScholesInputs(REF, r, float(S0), sigma)),
                       hh.CoxRossRubinsteinMethod(N)).price
        want = analytic.crr_price(S0, K, r, sigma, T, N, cp=cp, american=am, on_forward=fwd)
        u = math.exp(sigma * math.sqrt(T / N))
        ks = np.arange(-N, N + 1)
        delta_w = float(np.max(np.abs(node_factors(u, N) / u ** ks.astype(np.float64) - 1.0)))
        p = 1.0 / (1.0 + u)
        F = S0 / math.exp(-r * T)
        G = F * max(1.0, (p * u + (1.0 - p) / u) ** N)
        bound = delta_w * G + 7 * N * EPS * (G + K)
        rel = abs(got - want) / abs(want)
        worst = max(worst, rel)
        print(f"\nN={N} sigma={sigma} T={T:.3f}: device {got!r} oracle {want!r} |diff| {abs(got - want):.3e} "
              f"bound {bound:.3e} (delta_w {delta_w:.2e}) rel {rel:.2e}")
        assert abs(got - want) <= bound
        assert rel <= 1e-11
    print(f"worst relative deviation from the oracle: {worst:.3e}")


def test_a_mixed_basket_equals_single_solves():
    """>= 300 payoffs (strikes, expiries, styles, call/put, Spot/Forward) in ONE call: each == its own solve."""
    m = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.22)
    rng = np.random.default_rng(7)
    expiries = [hh.Date(2020, 3, 1), hh.Date(2020, 9, 15), hh.Date(2021, 1, 1), hh.Date(2022, 6, 30)]
    payoffs = []
    for n in range(320):
        ex, cp, und = ALL8[n % 8]
        payoffs.append(opt(float(rng.uniform(60, 140)), expiries[n % 4], ex, cp, und))
    meth = hh.CoxRossRubinsteinMethod(300)
    basket = hh.solve(hh.BasketPricingProblem(payoffs, m), meth)
    assert len(basket.solutions) == 320
    for p, s in zip(payoffs, basket.solutions):
        assert s.price == hh.solve(hh.PricingProblem(p, m), meth).price


def test_european_tree_agrees_with_black_scholes():
    """price_agreement.jl: CRR(100) against BlackScholesAnalytic, atol 1e-3 (its case, and two more)."""
    expiry = REF + __import__("datetime").timedelta(days=365)
    for spot, K, sigma, r in ((1.0, 1.0, 0.4, 0.2), (1.0, 1.2, 0.3, 0.02), (1.0, 0.8, 0.2, 0.0)):
        m = hh.BlackScholesInputs(REF, r, spot, sigma)
        for cp in (hh.Call(), hh.Put()):
            prob = hh.PricingProblem(opt(K, expiry, hh.European(), cp, hh.Spot()), m)
            tree = hh.solve(prob, hh.CoxRossRubinsteinMethod(100)).price
            bs = hh.solve(prob, hh.BlackScholesAnalytic()).price
            assert abs(tree - bs) <= 1e-3, (spot, K, sigma, r, cp, tree, bs)


def test_lsm_agrees_with_the_device_tree():
    """american_options.jl: LSM against solve(prob, CoxRossRubinsteinMethod(n)) at rtol 0.02 / 0.03."""
    def both(K, cp, expiry, r, spot, sigma, n, steps, degree, seed, tree_steps):
        m = hh.BlackScholesInputs(REF, r, spot, sigma)
        prob = hh.PricingProblem(opt(K, expiry, hh.American(), cp, hh.Spot()), m)
        cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(seed, seed + n))
        lsm = hh.solve(prob, hh.LSM(hh.LognormalDynamics(), hh.BlackScholesExact(), cfg, degree)).price
        return lsm, hh.solve(prob, hh.CoxRossRubinsteinMethod(tree_steps)).price

    lsm, tree = both(100.0, hh.Put(), hh.add_years(REF, 1), 0.05, 100.0, 0.2, 50_000, 100, 5, 12345, 1000)
    assert lsm == pytest.approx(tree, rel=0.02)
    lsm, tree = both(100.0, hh.Call(), hh.add_years(REF, 1), 0.15, 120.0, 0.3, 30_000, 100, 5, 54321, 800)
    assert lsm == pytest.approx(tree, rel=0.03)


def test_fd_delta_through_the_tree():
    """FDCentral delta via GreekProblem(prob, SpotLens()) == the restatement's FD delta within 1e-10."""
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.25)
    payoff = opt(100.0, hh.Date(2021, 1, 1), hh.American(), hh.Put(), hh.Spot())
    prob = hh.PricingProblem(payoff, m)
    fd = hh.FiniteDifference(1e-4, hh.FDCentral())
    got = hh.solve(hh.GreekProblem(prob, hh.SpotLens()), fd, hh.CoxRossRubinsteinMethod(500)).greek
    up = restated_prices([payoff], hh.BlackScholesInputs(REF, 0.05, 100.0 * (1 + 1e-4), 0.25), 500)[0]
    dn = restated_prices([payoff], hh.BlackScholesInputs(REF, 0.05, 100.0 * (1 - 1e-4), 0.25), 500)[0]
    want = (up - dn) / (2 * 1e-4 * 100.0)
    print(f"\nFD delta {got!r} (restatement {want!r})")
    assert abs(got - want) <= 1e-10 and -1.0 < got < 0.0
