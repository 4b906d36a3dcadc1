"""Device Carr–Madan against the scipy restatement (oracle/analytic.py) and the
values the reference's MC tests use as their targets."""
import numpy as np
import pytest

import hedgehog_jl_amd as hh
from oracle import analytic

pytestmark = pytest.mark.gpu


def heston_prob(params, r, ref, expiry, K=100.0, cp=None):
    payoff = hh.VanillaOption(K, expiry, hh.European(), cp or hh.Call(), hh.Spot())
    return hh.PricingProblem(payoff, hh.HestonInputs(ref, r, 100.0, *params))


TARGETS = [
    ((0.04, 2.0, 0.04, 0.3, -0.7), 0.03, hh.Date(2020, 1, 1), hh.Date(2021, 1, 1), 32.0,
     9.257069529912402),                                   # montecarlo_heston.jl:13-49
    ((0.04, 2.0, 0.04, 0.3, -0.7), 0.03, hh.Date(2021, 1, 1), hh.Date(2022, 1, 1), 400.0,
     9.242521073959068),                                   # H252
    ((1.5, 0.04, 0.3, -0.6, 0.04), 0.05, hh.Date(2025, 1, 1), hh.Date(2025, 12, 31), 32.0,
     46.31412390823014),                                   # montecarlo_heston.jl:161-170 as run (Q2)
]


@pytest.mark.parametrize("params,r,ref,expiry,bound,target", TARGETS)
def test_carr_madan_heston_targets(params, r, ref, expiry, bound, target):
    prob = heston_prob(params, r, ref, expiry)
    price = hh.solve(prob, hh.CarrMadan(1.0, bound, hh.HestonDynamics())).price
    assert price == pytest.approx(target, rel=1e-9)
    T = hh.yearfrac(ref, expiry)
    V0, k, th, s, rho = params
    assert price == pytest.approx(
        analytic.carr_madan_heston(100.0, 100.0, r, V0, k, th, s, rho, T, bound=bound), rel=1e-9)
    put = hh.solve(heston_prob(params, r, ref, expiry, cp=hh.Put()),
                   hh.CarrMadan(1.0, bound, hh.HestonDynamics())).price
    assert put == pytest.approx(price - 100.0 + 100.0 * np.exp(-r * T), rel=1e-12)


# TARGETS[0] (α = 1, bound 32: one sub-panel per lane) as the library returned it on an MI355X BEFORE the panels
# were cut into sub-panels (carr_madan_subpanels): the call through `solve`, through hh_carr_madan_basket, and from
# hh_carr_madan_basket_grad the price and its partials along S0, V0, κ, θ, σ, ρ, r_drift and the discount factor.
PLAIN_RULE_FIRST_TARGET = dict(
    solve="0x1.2839e9e0f8b2fp+3",
    basket="0x1.2839e9e0f8b2fp+3",
    grad=["0x1.2839e9e0f8b27p+3", "0x1.4fbc60344db94p-1", "0x1.45839eca422a1p+5",
          "0x1.5738dcfaba095p-4", "0x1.b96d848734801p+5", "-0x1.441d0484b5ffep+0",
          "0x1.d0613f2731828p-6", "0x1.07032228f961cp+6", "0x1.3145d2b65123fp+3"],
)


def first_target_on_the_device():
    params, r, ref, expiry, bound, _ = TARGETS[0]
    from hedgehog_jl_amd import _ffi
    T = hh.yearfrac(ref, expiry)
    V0, kappa, theta, sigma, rho = params
    kw = dict(S0=100.0, V0=V0, kappa=kappa, theta=theta, sigma=sigma, rho=rho)
    args = (hh.get_context(0), kw, _ffi.HH_HESTON, [100.0], [1.0], [T], [r])
    solve = hh.solve(heston_prob(params, r, ref, expiry), hh.CarrMadan(1.0, bound, hh.HestonDynamics())).price
    basket = _cm_basket(*args, bound=bound)
    gprice, grad = _cm_basket(*args, bound=bound, grad=True)
    return dict(solve=float(solve).hex(), basket=float(basket[0]).hex(),
                grad=[float(x).hex() for x in (gprice[0], *grad[0])])


def test_one_subpanel_per_lane_is_the_plain_rule_bit_for_bit():
    """m = 1 — every setting the reference itself uses — must compute what the rule without sub-panels computed, in
    all three kernels' shared panel loop: `==` on values recorded from the library before the loop was cut up."""
    got = first_target_on_the_device()
    assert got == PLAIN_RULE_FIRST_TARGET
    assert got["basket"] == got["solve"]


def test_carr_madan_lognormal_equals_black_scholes():
    """test/agreement/price_agreement.jl: Carr–Madan with the lognormal law vs BlackScholesAnalytic,
    atol 1e-6 (365-day expiry, so the √α quirk of montecarlo.jl:302 is invisible)."""
    ref = hh.Date(2021, 1, 1)
    for K in (80.0, 100.0, 125.0):
        for cp in (hh.Call(), hh.Put()):
            payoff = hh.VanillaOption(K, hh.Date(2022, 1, 1), hh.European(), cp, hh.Spot())
            prob = hh.PricingProblem(payoff, hh.BlackScholesInputs(ref, 0.05, 100.0, 0.2))
            cm = hh.solve(prob, hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics())).price
            bs = hh.solve(prob, hh.BlackScholesAnalytic()).price
            assert cm == pytest.approx(bs, abs=1e-6)
            assert bs == pytest.approx(analytic.bs_price(100.0, K, 0.05, 0.2, 1.0, cp()), rel=1e-13)


def test_monte_carlo_against_the_device_fourier_price():
    """The reference's Heston agreement test, entirely on the GPU box: Euler MC vs device Carr–Madan."""
    prob = heston_prob((0.04, 2.0, 0.04, 0.3, -0.7), 0.03, hh.Date(2020, 1, 1), hh.Date(2021, 1, 1))
    cm = hh.solve(prob, hh.CarrMadan(1.0, 32.0, hh.HestonDynamics())).price
    n = 400_000
    mc = hh.solve(prob, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                                      hh.SimulationConfig(n, steps=200, seeds=np.arange(1, n + 1),
                                                          variance_reduction=hh.Antithetic())),
                  ensemble=False)
    assert abs(mc.price - cm) < 4 * mc.std_error + 0.02


try:
    from hypothesis import HealthCheck, Phase, given, settings
    from hypothesis import strategies as st
except ImportError:  # pragma: no cover
    given = None

if given is not None:
    @settings(max_examples=60, deadline=None, derandomize=True, database=None,
              phases=[Phase.explicit, Phase.generate], suppress_health_check=[HealthCheck.too_slow])
    @given(V0=st.floats(0.005, 0.5), kappa=st.floats(0.1, 5.0), theta=st.floats(0.005, 0.3),
           sigma=st.floats(0.05, 1.2), rho=st.floats(-0.95, 0.95), r=st.floats(-0.01, 0.1),
           days=st.integers(20, 1500), moneyness=st.floats(0.6, 1.6), alpha=st.sampled_from([0.25, 0.75, 1.0, 1.5]),
           bound=st.sampled_from([32.0, 100.0, 400.0, 1000.0]), put=st.booleans())
    def test_carr_madan_random_heston(V0, kappa, theta, sigma, rho, r, days, moneyness, alpha, bound, put):
        """Random Heston parameters, damping and integration bounds: the device quadrature against the
        scipy restatement of carr_madan.jl:47-92 (same integrand, adaptive quadrature).  Absolute bar
        1e-7 of the spot: the reference itself compares the method to others with atol 1e-6 … 1e-2."""
        import datetime as dt
        ref = hh.Date(2021, 1, 1)
        expiry = ref + dt.timedelta(days=days)
        K = 100.0 * moneyness
        prob = heston_prob((V0, kappa, theta, sigma, rho), r, ref, expiry, K=K, cp=hh.Put() if put else hh.Call())
        price = hh.solve(prob, hh.CarrMadan(alpha, bound, hh.HestonDynamics())).price
        T = hh.yearfrac(ref, expiry)
        want = analytic.carr_madan_heston(100.0, K, r, V0, kappa, theta, sigma, rho, T, alpha=alpha, bound=bound)
        if put:
            want = want - 100.0 + K * np.exp(-r * T)
        assert np.isfinite(price)
        assert price == pytest.approx(want, abs=1e-5)


def test_carr_madan_basket_equals_single_solves():
    """solve(::BasketPricingProblem, ::CarrMadan): every Fourier integral of the basket in one launch
    (the calibration objective's inner loop, calibration.jl:75-88) equals the per-payoff solves bit for
    bit — same integrand, same panels, same reduction — over strikes, expiries, calls and puts."""
    ref = hh.Date(2021, 1, 1)
    mkt = hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)
    payoffs = [hh.VanillaOption(K, e, hh.European(), cp, hh.Spot())
               for e in (hh.Date(2021, 4, 1), hh.Date(2022, 1, 1), hh.Date(2024, 1, 1))
               for K in (70.0, 95.0, 100.0, 130.0) for cp in (hh.Call(), hh.Put())]
    method = hh.CarrMadan(1.0, 32.0, hh.HestonDynamics())
    sol = hh.solve(hh.BasketPricingProblem(payoffs, mkt), method)
    assert isinstance(sol, hh.BasketPricingSolution) and len(sol.solutions) == len(payoffs)
    for p, s in zip(payoffs, sol.solutions):
        assert s.price == hh.solve(hh.PricingProblem(p, mkt), method).price
        assert s.problem.payoff is p
    # the lognormal law, with the reference's √T quirk on and off (366-day expiry: they differ)
    bs = hh.BlackScholesInputs(ref, 0.05, 100.0, 0.2)
    pays = [hh.VanillaOption(K, hh.Date(2022, 1, 2), hh.European(), hh.Call(), hh.Spot()) for K in (90.0, 110.0)]
    for compat in (False, True):
        meth = hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics(), compat_sqrt_alpha=compat)
        got = [s.price for s in hh.solve(hh.BasketPricingProblem(pays, bs), meth).solutions]
        assert got == [hh.solve(hh.PricingProblem(p, bs), meth).price for p in pays]


def _cm_basket(ctx, model_kw, dyn, strikes, cps, Ts, rs, alpha=1.0, bound=32.0, grad=False, compat=0):
    import ctypes as C
    from hedgehog_jl_amd import _ffi
    m = _ffi.make_model(**model_kw)
    K = len(strikes)
    strikes, cps, Ts, rs = (np.ascontiguousarray(x, dtype=np.float64) for x in (strikes, cps, Ts, rs))
    Ds = np.exp(-rs * Ts)
    out, g = np.empty(K), np.empty((K, _ffi.HH_CM_GRAD_LEN))
    args = (ctx.handle, C.byref(m), dyn, compat, alpha, bound, strikes.ctypes.data, cps.ctypes.data,
            Ts.ctypes.data, rs.ctypes.data, Ds.ctypes.data, K, out.ctypes.data)
    if grad:
        ctx.check(ctx.lib.hh_carr_madan_basket_grad(*args, g.ctypes.data))
        return out, g
    ctx.check(ctx.lib.hh_carr_madan_basket(*args))
    return out


@pytest.mark.parametrize("dyn", ["heston", "lognormal"])
def test_carr_madan_gradient_against_finite_differences(dyn):
    """hh_carr_madan_basket_grad — what ForwardDiff pushes through carr_madan.jl:47-92 / heston.jl:307-319
    for a differentiated calibration objective — against central differences of the device prices
    (same quadrature: only the differentiation differs) and, for Heston, of the scipy restatement."""
    from hedgehog_jl_amd import _ffi
    ctx = hh.get_context(0)
    base = dict(S0=100.0, V0=0.05, kappa=1.7, theta=0.06, sigma=0.45, rho=-0.6) if dyn == "heston" else \
        dict(S0=100.0, sigma=0.25)
    code = _ffi.HH_HESTON if dyn == "heston" else _ffi.HH_LOGNORMAL
    strikes = np.array([70.0, 95.0, 100.0, 120.0, 100.0, 90.0])
    cps = np.array([1.0, 1.0, -1.0, 1.0, 1.0, -1.0])
    Ts = np.array([0.25, 1.0, 1.0, 2.5, 0.5, 3.0])
    rs = np.array([0.01, 0.03, 0.03, 0.035, 0.02, 0.04])
    price, grad = _cm_basket(ctx, base, code, strikes, cps, Ts, rs, grad=True)
    np.testing.assert_allclose(price, _cm_basket(ctx, base, code, strikes, cps, Ts, rs), rtol=1e-13)
    slots = {"S0": 0, "V0": 1, "kappa": 2, "theta": 3, "sigma": 4, "rho": 5}
    for name, j in slots.items():
        if name not in base:
            assert np.all(grad[:, j] == 0.0)
            continue
        h = 1e-5 * max(abs(base[name]), 0.1)
        up = _cm_basket(ctx, dict(base, **{name: base[name] + h}), code, strikes, cps, Ts, rs)
        dn = _cm_basket(ctx, dict(base, **{name: base[name] - h}), code, strikes, cps, Ts, rs)
        fd = (up - dn) / (2 * h)
        np.testing.assert_allclose(grad[:, j], fd, rtol=2e-6, atol=2e-7, err_msg=name)
    # the rate enters through r_drift (slot 6) and the discount factor (slot 7): flat curve, both at once
    h = 1e-6
    Dup, Ddn = np.exp(-(rs + h) * Ts), np.exp(-(rs - h) * Ts)
    up = _cm_basket(ctx, base, code, strikes, cps, Ts, rs + h)
    dn = _cm_basket(ctx, base, code, strikes, cps, Ts, rs - h)
    total = grad[:, 6] + grad[:, 7] * (-Ts * np.exp(-rs * Ts))
    np.testing.assert_allclose(total, (up - dn) / (2 * h), rtol=2e-6, atol=2e-7)
    assert np.all(Dup < Ddn)
    if dyn == "heston":  # an independent quadrature: scipy, adaptive
        k = 1
        f = lambda **kw: analytic.carr_madan_heston(100.0, strikes[k], rs[k], **{**dict(V0=0.05, kappa=1.7, theta=0.06, sigma=0.45, rho=-0.6), **kw}, T=Ts[k])
        for name, j in (("V0", 1), ("kappa", 2), ("theta", 3), ("sigma", 4), ("rho", 5)):
            h = 1e-4 * abs(base[name])
            fd = (f(**{name: base[name] + h}) - f(**{name: base[name] - h})) / (2 * h)
            assert grad[k, j] == pytest.approx(fd, rel=1e-5, abs=1e-6), name


def test_carr_madan_basket_returns_dual_prices():
    """solve(::BasketPricingProblem, ::CarrMadan) on Dual inputs — the calibration objective under
    AutoForwardDiff (calibration.jl:75-88): the prices come back as Duals whose partials are the
    device gradient contracted with the seeds, rate curve included."""
    from hedgehog_jl_amd.dual import Dual
    ref = hh.Date(2021, 1, 1)
    e = lambda j: tuple(1.0 if i == j else 0.0 for i in range(4))
    x = dict(V0=0.05, kappa=1.7, sigma=0.45, r=0.03)
    mkt = lambda **kw: hh.HestonInputs(ref, kw.get("r", x["r"]), 100.0, kw.get("V0", x["V0"]),
                                       kw.get("kappa", x["kappa"]), 0.06, kw.get("sigma", x["sigma"]), -0.6)
    payoffs = [hh.VanillaOption(K, ex, hh.European(), cp, hh.Spot())
               for K, ex, cp in ((90.0, hh.Date(2022, 1, 1), hh.Call()), (105.0, hh.Date(2021, 7, 1), hh.Put()),
                                 (100.0, hh.Date(2023, 1, 1), hh.Call()))]
    method = hh.CarrMadan(1.0, 32.0, hh.HestonDynamics())
    seeded = mkt(V0=Dual(x["V0"], e(0)), kappa=Dual(x["kappa"], e(1)), sigma=Dual(x["sigma"], e(2)),
                 r=Dual(x["r"], e(3)))
    sol = hh.solve(hh.BasketPricingProblem(payoffs, seeded), method)
    plain = hh.solve(hh.BasketPricingProblem(payoffs, mkt()), method)
    for j, name in enumerate(("V0", "kappa", "sigma", "r")):
        h = 1e-5 * max(abs(x[name]), 0.1)
        up = hh.solve(hh.BasketPricingProblem(payoffs, mkt(**{name: x[name] + h})), method)
        dn = hh.solve(hh.BasketPricingProblem(payoffs, mkt(**{name: x[name] - h})), method)
        for s, p0, u, d in zip(sol.solutions, plain.solutions, up.solutions, dn.solutions):
            assert isinstance(s.price, Dual) and s.price.value == pytest.approx(p0.price, rel=1e-13)
            assert s.price.partials[j] == pytest.approx((u.price - d.price) / (2 * h), rel=5e-6, abs=5e-7), name


if given is not None:
    @settings(max_examples=40, deadline=None, derandomize=True, database=None,
              phases=[Phase.explicit, Phase.generate], suppress_health_check=[HealthCheck.too_slow])
    @given(V0=st.floats(0.01, 0.4), kappa=st.floats(0.2, 5.0), theta=st.floats(0.01, 0.3),
           sigma=st.floats(0.1, 1.0), rho=st.floats(-0.9, 0.9), r=st.floats(0.0, 0.08),
           T=st.floats(0.1, 4.0), moneyness=st.floats(0.7, 1.4), put=st.booleans())
    def test_carr_madan_gradient_random_heston(V0, kappa, theta, sigma, rho, r, T, moneyness, put):
        """The device gradient over random Heston parameters against central differences of the device
        prices: the complex logarithm and square root of the CF stay on their branches (the formulation
        with exp(-d1 T) of heston.jl:307-319) and so do their partials."""
        from hedgehog_jl_amd import _ffi
        ctx = hh.get_context(0)
        base = dict(S0=100.0, V0=V0, kappa=kappa, theta=theta, sigma=sigma, rho=rho)
        args = (np.array([100.0 * moneyness]), np.array([-1.0 if put else 1.0]), np.array([T]), np.array([r]))
        price, grad = _cm_basket(ctx, base, _ffi.HH_HESTON, *args, grad=True)
        assert np.isfinite(price[0]) and np.all(np.isfinite(grad))
        for name, j in (("S0", 0), ("V0", 1), ("kappa", 2), ("theta", 3), ("sigma", 4), ("rho", 5)):
            h = 2e-5 * max(abs(base[name]), 0.05)
            up = _cm_basket(ctx, dict(base, **{name: base[name] + h}), _ffi.HH_HESTON, *args)[0]
            dn = _cm_basket(ctx, dict(base, **{name: base[name] - h}), _ffi.HH_HESTON, *args)[0]
            fd = (up - dn) / (2 * h)
            scale = max(abs(fd), abs(price[0]) / max(abs(base[name]), 0.05), 1e-2)
            assert abs(grad[0, j] - fd) <= 2e-5 * scale, (name, grad[0, j], fd)


def test_heston_calibration_scenario_of_the_reference():
    """test/unit/calibration.jl:38-108 on the device path: 51 Carr–Madan quotes from known Heston
    parameters, start and bounds as there; the reference asks for each parameter within rtol 1e-1 — with
    the exact Jacobian from the device the fit is to 1e-4."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location(
        "heston_calibration", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           "examples", "heston_calibration.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, sse, evals, wall = mod.calibrate()
    np.testing.assert_allclose(x, mod.TRUE, rtol=1e-4)
    assert sse < 1e-12 and evals < 200


def test_ad_greeks_through_carr_madan():
    """solve(GreekProblem(prob, lens), ForwardAD(), CarrMadan(...)) (greeks_problem.jl:249-262): the Dual the
    lens plants reaches the device as a gradient request and comes back as the price's partial — Δ, ∂V0
    and ρ (drift and discount together, through the rate curve) of the H252 problem, against the values
    the Monte Carlo Greek tests use as their Fourier targets, and against finite differences."""
    prob = heston_prob((0.04, 2.0, 0.04, 0.3, -0.7), 0.03, hh.Date(2021, 1, 1), hh.Date(2022, 1, 1))
    method = hh.CarrMadan(1.0, 400.0, hh.HestonDynamics())
    lenses = (hh.optic("market_inputs.spot"), hh.optic("market_inputs.V0"), hh.optic("market_inputs.rate.rate"))
    targets = (0.65565115, 40.7248418, 56.3225943)
    for lens, want in zip(lenses, targets):
        g = hh.solve(hh.GreekProblem(prob, lens), hh.ForwardAD(), method).greek
        assert g == pytest.approx(want, rel=2e-7)
        fd = hh.solve(hh.GreekProblem(prob, lens), hh.FiniteDifference(1e-5), method).greek
        assert g == pytest.approx(fd, rel=1e-6)
    batch = hh.solve(hh.BatchGreekProblem(prob, lenses), hh.ForwardAD(), method)
    assert [batch[l] for l in lenses] == pytest.approx(list(targets), rel=2e-7)
