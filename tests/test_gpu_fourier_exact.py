"""Device Carr–Madan (hh_fourier.hip) against the exact truncated integral (tests/golden/carr_madan_exact.json:
mpmath at 50 digits, oracle/carr_madan_exact.py): the price from all three entry points, all eight slots of the
gradient, and the same prices through `hh.solve` with dates, on every golden case.  The bars are
tests/carr_madan_cases.py's: a floor of rounding size or 20× what fp64 rounding alone costs on that case (`e64`),
neither taken from the device.  The plain 256-panel rule misses these bars wherever bound/256 ≥ 1.56·α
(tests/test_carr_madan_exact_host.py); the sub-panels of `carr_madan_subpanels` are what meets them.  The module
prints its worst error/bar per kind of comparison at its end (`-s`)."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests.carr_madan_cases import BY_ID, GOLDEN, GRAD_SLOTS, err, exact_price, grad_bar, price_bar

pytestmark = pytest.mark.gpu

IDS = [r["id"] for r, _ in GOLDEN]
GRAD_IDS = [r["id"] for r, _ in GOLDEN if "grad" in r]


def _model(c):
    kw = dict(S0=c["S0"], sigma=c["sigma"], r=c["r_drift"], T=c["T"], strike=c["K"], discount=c["discount"])
    if c["dynamics"] == "heston":
        kw.update(V0=c["V0"], kappa=c["kappa"], theta=c["theta"], rho=c["rho"])
    return kw


def _device_results(ctx, c):
    """One case through the three entry points: the single solve as a call and as a put, and a basket of (call, put)
    with and without the gradient — one launch each, one workgroup per payoff."""
    dyn = _ffi.HH_HESTON if c["dynamics"] == "heston" else _ffi.HH_LOGNORMAL
    compat, kw = int(c["compat_sqrt_alpha"]), _model(c)
    single = {}
    for cp in (1.0, -1.0):
        out = C.c_double()
        m = _ffi.make_model(cp=cp, **kw)
        ctx.check(ctx.lib.hh_carr_madan(ctx.handle, C.byref(m), dyn, compat, c["alpha"], c["bound"], C.byref(out)))
        single[cp] = out.value
    m = _ffi.make_model(**kw)
    arrs = [np.array([x, x]) for x in (c["K"],)] + [np.array([1.0, -1.0])] + \
           [np.array([x, x]) for x in (c["T"], c["r_drift"], c["discount"])]
    basket, gprice, grad = np.empty(2), np.empty(2), np.empty((2, _ffi.HH_CM_GRAD_LEN))
    args = (ctx.handle, C.byref(m), dyn, compat, c["alpha"], c["bound"], *[a.ctypes.data for a in arrs], 2)
    ctx.check(ctx.lib.hh_carr_madan_basket(*args, basket.ctypes.data))
    ctx.check(ctx.lib.hh_carr_madan_basket_grad(*args, gprice.ctypes.data, grad.ctypes.data))
    return dict(single=single, basket={1.0: basket[0], -1.0: basket[1]}, gprice={1.0: gprice[0], -1.0: gprice[1]},
                grad=grad)


@pytest.fixture(scope="module")
def device():
    ctx = hh.get_context(0)
    return {r["id"]: _device_results(ctx, c) for r, c in GOLDEN}


@pytest.fixture(scope="module")
def worst():
    """error/bar of every comparison made, for the line the module prints at its end."""
    w = {}
    yield w
    for k, (ratio, where) in sorted(w.items()):
        print(f"\ncarr_madan_exact worst error/bar, {k}: {ratio:.3g} ({where})")


def _note(worst, key, ratio, where):
    if ratio > worst.get(key, (-1.0, ""))[0]:
        worst[key] = (ratio, where)


@pytest.mark.parametrize("name", IDS)
def test_prices_against_the_exact_integral(device, worst, name):
    r, c = BY_ID[name]
    d, bar = device[name], price_bar(r, c)
    for cp in (1.0, -1.0):
        want = exact_price(r, c, cp)
        for entry in ("single", "basket", "gprice"):
            _note(worst, "price", err(d[entry][cp], want) / bar, f"{name} {entry} cp={cp:+.0f}")
    for cp in (1.0, -1.0):
        assert d["basket"][cp] == d["single"][cp], (name, cp)     # same integrand, panels and reduction: bit for bit
        for entry in ("single", "basket", "gprice"):
            assert err(d[entry][cp], exact_price(r, c, cp)) <= bar, (name, entry, cp)


@pytest.mark.parametrize("name", GRAD_IDS)
def test_gradient_against_the_exact_gradient(device, worst, name):
    """All eight slots of the call's gradient; the put's differ by parity in S0 (−1) and the discount (+K) exactly."""
    import mpmath as mp
    r, c = BY_ID[name]
    got, bar = device[name]["grad"], grad_bar(r, c)
    errs = np.array([err(got[0, j], mp.mpf(r["grad"][j])) for j in range(len(GRAD_SLOTS))])
    for j, slot in enumerate(GRAD_SLOTS):
        _note(worst, "gradient", errs[j] / bar[j], f"{name} {slot}")
    if c["dynamics"] == "lognormal":
        assert all(got[0, j] == 0.0 for j in (1, 2, 3, 5))
    assert np.all(errs <= bar), dict(zip(GRAD_SLOTS, errs / bar))
    shift = np.zeros(len(GRAD_SLOTS))
    shift[0], shift[7] = -1.0, c["K"]
    np.testing.assert_allclose(got[1], got[0] + shift, rtol=0, atol=4 * np.finfo(float).eps * np.abs(got[0]).max())


@pytest.mark.parametrize("name", IDS)
def test_solve_with_dates_against_the_exact_integral(worst, name):
    """The parameter seam: `hh.solve(PricingProblem, CarrMadan(α, bound, …))` forms T, r_drift, the discount factor and
    compat_sqrt_alpha on the host (flat curve at the case's rate, expiry `days` after the reference date)."""
    r, c = BY_ID[name]
    ref = hh.Date(2021, 1, 1)
    expiry = ref + dt.timedelta(days=r["days"])
    assert hh.yearfrac(ref, expiry) == c["T"]
    if c["dynamics"] == "heston":
        mkt = hh.HestonInputs(ref, c["r_drift"], c["S0"], c["V0"], c["kappa"], c["theta"], c["sigma"], c["rho"])
        method = hh.CarrMadan(c["alpha"], c["bound"], hh.HestonDynamics())
    else:
        mkt = hh.BlackScholesInputs(ref, c["r_drift"], c["S0"], c["sigma"])
        method = hh.CarrMadan(c["alpha"], c["bound"], hh.LognormalDynamics(), compat_sqrt_alpha=c["compat_sqrt_alpha"])
    bar = price_bar(r, c)
    for cp, side in ((1.0, hh.Call()), (-1.0, hh.Put())):
        payoff = hh.VanillaOption(c["K"], expiry, hh.European(), side, hh.Spot())
        price = hh.solve(hh.PricingProblem(payoff, mkt), method).price
        e = err(price, exact_price(r, c, cp))
        _note(worst, "solve", e / bar, f"{name} cp={cp:+.0f}")
        assert e <= bar, (name, cp)
