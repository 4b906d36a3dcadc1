"""The exact Carr–Madan reference (oracle/carr_madan_exact.py) and its golden file, checked on the CPU: against
closed forms and an independent Fourier representation, for the branch of the Heston logarithm, for the
size of fp64 rounding (`e64`), and — the finding the device tests rest on — that the plain 256-panel rule
misses the exact integral once a panel's half-width h = bound/256 is large against the damping α."""
import importlib.util
import os

import mpmath as mp
import numpy as np
import pytest

from oracle import carr_madan_exact as exact
from oracle import carr_madan_fp64 as fp64

from tests.carr_madan_cases import BY_ID, GOLDEN, GOLDEN_DIR, GRAD_FLOOR, grad_scale, price_bar


def _ncdf(x):
    return mp.erfc(-x / mp.sqrt(2)) / 2


def lognormal_law_price(c):
    """The call on S_T with log S_T ~ Normal(μ, s²): D·(e^{μ+s²/2}·N(d1) − K·N(d2)) — Black–Scholes when μ = log S0 +
    (r − σ²/2)T; the put from it by the parity the entry points apply, −S0 + K·D (D is a given number here, not
    e^{−rT} to 40 digits, so the closed put would differ in the 16th digit)."""
    S0, K, T, r, D, sig = (mp.mpf(c[k]) for k in ("S0", "K", "T", "r_drift", "discount", "sigma"))
    s = sig * mp.sqrt(T)
    mu = mp.log(S0) + (r - sig * sig / 2) * (mp.sqrt(T) if c["compat_sqrt_alpha"] else T)
    d2 = (mu - mp.log(K)) / s
    d1 = d2 + s
    call = D * (mp.exp(mu + s * s / 2) * _ncdf(d1) - K * _ncdf(d2))
    return call if c["cp"] > 0 else call - S0 + K * D


def test_lognormal_integral_equals_the_closed_form():
    """σ√T·bound ≥ 12: the integrand beyond the bound is below e^{−72}/v², the truncated tail below 1e-30, so the
    exact truncated integral IS the closed price.  The golden values, and one integral computed here."""
    n = 0
    with mp.workdps(40):
        for r, c in GOLDEN:
            if r["dynamics"] != "lognormal" or c["sigma"] * np.sqrt(c["T"]) * c["bound"] < 12.0:
                continue
            assert abs(mp.mpf(r["price"]) - lognormal_law_price(c)) < mp.mpf("1e-25"), r["id"]
            n += 1
        assert n >= 6
        for name in ("ln_730d_compat", "ln_K100_put"):
            c = BY_ID[name][1]
            assert abs(exact.price(c) - lognormal_law_price(c)) < mp.mpf("1e-25")


def _heston_cf_real_line(c, u):
    """ϕ(u) of log S_T, written out again (Albrecher et al. form) for the Gil-Pelaez integrals."""
    kappa, theta, sigma, rho, V0, T = (mp.mpf(c[k]) for k in ("kappa", "theta", "sigma", "rho", "V0", "T"))
    x = mp.log(mp.mpf(c["S0"])) + mp.mpf(c["r_drift"]) * T
    b = kappa - rho * sigma * 1j * u
    d = mp.sqrt(b * b + sigma ** 2 * (1j * u + u * u))
    g = (b - d) / (b + d)
    e = mp.exp(-d * T)
    A = kappa * theta / sigma ** 2 * ((b - d) * T - 2 * mp.log((1 - g * e) / (1 - g)))
    B = (b - d) / sigma ** 2 * (1 - e) / (1 - g * e)
    return mp.exp(A + B * V0 + 1j * u * x)


@pytest.mark.parametrize("name", ["gil_pelaez_K90", "gil_pelaez_K120"])
def test_heston_integral_equals_gil_pelaez(name):
    """call = D·(F·P1 − K·P2), P_j = 1/2 + (1/π)∫_0^∞ Re(e^{−iu log K} ϕ_j(u)/(iu)) du, ϕ_2 = ϕ, ϕ_1(u) = ϕ(u − i)/ϕ(−i),
    F = ϕ(−i): no damping, no pole off the axis, another contour.  |ϕ(u)| ≤ e^{−1.29·u}·const for these parameters
    ((V0 + κθT)·sqrt(1−ρ²)/σ = 1.30), so both this integral cut at 100 and the Carr–Madan one at bound 100 are
    within 1e-50 of their limits; 30 digits carried, 1e-22·S0 asked."""
    r, c = BY_ID[name]
    with mp.workdps(30):
        logK, F = mp.log(mp.mpf(c["K"])), _heston_cf_real_line(c, mp.mpc(0, -1)).real
        pts = [mp.mpf(0)] + [mp.mpf(2) ** k for k in range(-3, 1)] + [mp.mpf(x) for x in range(2, 101, 2)]
        P = []
        for cf in (lambda u: _heston_cf_real_line(c, u - 1j) / F, lambda u: _heston_cf_real_line(c, u)):
            f = lambda u, cf=cf: (mp.exp(-1j * u * logK) * cf(u) / (1j * u)).real
            P.append(mp.mpf(1) / 2 + mp.quad(f, pts) / mp.pi)
        call = mp.mpf(c["discount"]) * (F * P[0] - mp.mpf(c["K"]) * P[1])
        want = call if c["cp"] > 0 else call - mp.mpf(c["S0"]) + mp.mpf(c["K"]) * mp.mpf(c["discount"])
        assert abs(mp.mpf(r["price"]) - want) < mp.mpf("1e-22") * c["S0"]


def test_the_principal_logarithm_is_the_continuous_one():
    """Every Heston golden case: continuing log((1 − g e^{−d₁T})/(1 − g)) from v = 0 along the contour never leaves the
    principal sheet — the branch the device takes with atan2 is the right one on all of them."""
    assert all(r["max_sheet"] == 0 for r, _ in GOLDEN)
    assert sum(r["dynamics"] == "heston" for r, _ in GOLDEN) >= 30


def test_golden_file_is_what_the_generator_computes():
    spec = importlib.util.spec_from_file_location("make_carr_madan_exact",
                                                  os.path.join(GOLDEN_DIR, "make_carr_madan_exact.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert {c["id"] for c in gen.cases()} == set(BY_ID)
    assert gen.check({"a0.1_b16", "a1_b16", "ln_K125"}, workers=1) == []


def test_fp64_rounding_is_small_on_the_golden_cases():
    """e64 = |complex128 on a converged rule − exact|: at most 1e-9·S0 anywhere, and above 1e-12·S0 on at most four
    cases (vol of vol 0.001 and 0.01, where C = κθ/σ²·(…) cancels)."""
    e = {r["id"]: float(r["e64"]) / c["S0"] for r, c in GOLDEN}
    assert max(e.values()) <= 1e-9, e
    assert sum(x > 1e-12 for x in e.values()) <= 4, {k: x for k, x in e.items() if x > 1e-12}
    # e64 is rounding only if the rule it was measured on had converged: doubling its panels moved nothing above
    # 1e-15·S0 (with a gradient: 1e-15 of each partial's scale) — on every case but the four that cancel
    unsettled = [r["id"] for r, c in GOLDEN if r["settle"] > 1e-15]
    assert all(r["settle"] <= 1e-12 for r, _ in GOLDEN)
    assert len(unsettled) <= 4 and all(abs(BY_ID[k][1]["sigma"]) <= 0.01 for k in unsettled), unsettled
    # the gradient's bar of 1e-11·scale stands only if fp64 rounding alone stays 20× under it (measured: 2.4e-15·scale)
    n = 0
    for r, c in GOLDEN:
        if "grad" in r:
            assert len(r["grad"]) == len(r["e64_grad"]) == len(fp64.GRAD_SLOTS)
            e = np.array([float(x) for x in r["e64_grad"]]) / grad_scale(c, [mp.mpf(g) for g in r["grad"]])
            assert e.max() <= GRAD_FLOOR / 20, (r["id"], e)
            n += 1
    assert n >= 12


def test_plain_256_panel_rule_misses_where_h_over_alpha_is_large():
    """The rule without sub-panels (m = 1) against the exact integral.  The damped transform's pole at v = iα has
    residue ∝ S0 whatever the model, so the miss depends on h/α alone, h = bound/256:
      h/α ≤ 0.78: within 1e-12·S0 — and the rule the kernel now uses (m = subpanels(α, bound)) meets the device
      tests' own bar everywhere, in numpy;
      h/α ≥ 1.56: off by more than 5e-13·S0 — 50× the floor of the device tests' bar (1e-14·S0), so those cannot pass
      on the plain rule — growing to 1e-10·S0 by h/α = 3 and to percents of the spot by h/α = 40."""
    seen = {"small": 0, "large": 0}
    for r, c in GOLDEN:
        call = float(mp.mpf(r["price"]) - (0 if c["cp"] > 0 else -mp.mpf(c["S0"]) + mp.mpf(c["K"]) * mp.mpf(c["discount"])))
        e64 = float(r["e64"])
        ratio = c["bound"] / 256 / c["alpha"]
        miss = abs(fp64.fixed_rule(c, 1) - call)
        fixed = abs(fp64.fixed_rule(c, fp64.subpanels(c["alpha"], c["bound"])) - call)
        assert fixed <= price_bar(r, c), (r["id"], fixed)
        if ratio <= 0.78:
            assert miss <= max(1e-12 * c["S0"], 20 * e64), (r["id"], ratio, miss)
            seen["small"] += 1
        elif ratio >= 1.56:
            # 1e-10·S0 cannot be asked from 1.56 on: the miss there is 6.24e-11 at S0 = 100, i.e. 6.2e-13·S0
            # (target_h252, a0.25_b100, a1_b400_far_otm; 1.56e-9 at S0 = 2500) — the pole's S0·f(h/α) crosses 1e-10·S0 only near h/α = 3
            assert miss > 5e-13 * c["S0"], (r["id"], ratio, miss)
            if ratio >= 3.0:
                assert miss > 1e-10 * c["S0"], (r["id"], ratio, miss)
            seen["large"] += 1
    assert seen["small"] >= 15 and seen["large"] >= 15


def test_the_shared_rule_restatement_computes_what_the_three_copies_did():
    """tests/carr_madan_law_cases.cm_rule_fp64 on the 256-panel rule under each law's phi, against the doubles that
    merton_cases, vg_cases and bates_cases returned from their own copies of the frame before it was stated once
    (tests/golden/carr_madan_rule_fp64.json, float.hex()): every case of bates_cases.cm_cases() and every payoff of the
    Carr–Madan records of merton_exact.json and vg_exact.json, ==."""
    import json

    from tests import bates_cases as bt
    from tests import carr_madan_law_cases as cl
    from tests import merton_cases as mc
    from tests import vg_cases as vc
    want = json.load(open(os.path.join(GOLDEN_DIR, "carr_madan_rule_fp64.json")))
    got = {"bates": {key: cl.cm_rule_fp64(case, fp64.PANELS, bt.phi).hex() for key, case in bt.cm_cases().items()}}
    for law, mod in (("merton", mc), ("vg", vc)):
        got[law] = {}
        for rec in mod.load_golden()["carr_madan"]:
            for k, p in enumerate(rec["payoffs"]):
                case = cl.cm_case(dict(rec["model"], T=p["T"]), p["K"], rec["alpha"], rec["bound"], p["cp"])
                got[law][f"{rec['id']}/{k}"] = cl.cm_rule_fp64(case, fp64.PANELS, mod.phi).hex()
    assert {law: len(v) for law, v in got.items()} == {"bates": 5, "merton": 37, "vg": 24}
    assert got == want
