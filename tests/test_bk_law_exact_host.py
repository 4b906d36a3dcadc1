"""The exact conditional law of ∫V (oracle/bk_law_exact.py, tests/golden/bk_law_exact.json) checked against itself, and
the fp64 Broadie–Kaya oracle's samples held to it at the bars of tests/bk_law_exact_cases.py — the bars the device tests
use, shown here to be within reach of a correct implementation in doubles, in every one of the eight readings of the
root search (bk_law_exact_cases.READINGS).  No GPU.  Prints its worst residual/bar per reading, regime and control set
(`-s`)."""
import functools
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from oracle import bk_law_exact as bx  # noqa: E402
from oracle import bk_oracle  # noqa: E402
from tests import bk_law_exact_cases as bc  # noqa: E402

TEN = mp.mpf(10)
CHEAP = [rec["id"] for rec in bc.DOC["laws"] if rec["terms"] <= 160]  # laws whose table is rebuilt here: about a second each


def law_by_id(law_id):
    rec = bc.LAWS[law_id]
    p = bc.REGIMES[rec["regime"]]
    return rec, bx.Law(p["V0"], rec["VT"], p["kappa"], p["theta"], p["sigma"], p["T"])


def test_the_fixture_holds_the_cases_asked_for():
    from tests.test_gpu_bk import PARAMS
    assert bc.REGIMES == PARAMS and len(PARAMS) == 9
    for name in PARAMS:
        cs = [c for c in bc.cases_of(name) if c["VT"] != bx.VT_FLOOR and not bc.is_far(c)]
        assert len(cs) >= 6 and len({c["VT"] for c in cs}) == 3
        assert {c["u"] for c in cs} == {1e-3, 0.3, 0.5, 0.9, 0.999}
        assert abs(PARAMS[name]["rho"] * PARAMS[name]["kappa"] / PARAMS[name]["sigma"] - 0.5) >= 0.5
    absorbed = [c for c in bc.CASES if c["VT"] == bx.VT_FLOOR]
    assert absorbed and all(4 * bc.REGIMES[c["regime"]]["kappa"] * bc.REGIMES[c["regime"]]["theta"]
                            / bc.REGIMES[c["regime"]]["sigma"] ** 2 < 0.2 for c in absorbed)
    assert bc.CONTROLS["shipped"] == dict(bk_atol=1e-4, bk_cf_tol=1e-3, bk_n_sigma=5.0, bk_moment_h=1e-2,
                                          bk_newton_maxiter=10, bk_bisect_maxiter=100)
    t = bc.CONTROLS["tight"]
    assert (t["bk_atol"], t["bk_cf_tol"], t["bk_n_sigma"]) == (1e-10, 1e-10, 12.0)
    assert all(set(c["controls"]) == set(bc.CONTROLS) for c in bc.CASES)
    assert sum(not bc.is_far(c) for c in bc.CASES) == 84
    far = [c for c in bc.CASES if bc.is_far(c)]
    # (10⁻⁵ where the maker had to move a 10⁻⁶ inward: its docstring)
    assert sorted((c["regime"], c["u"]) for c in far) == sorted(
        (r, u) for r, low in (("h252", 1e-6), ("intended", 1e-5), ("nu_one", 1e-5)) for u in (low, 1 - 1e-6))
    assert [c for c in far if c["u"] < 0.5] == bc.FAR_LOW and len(bc.FAR_LOW) == 3
    for c in far:  # the regime's median V_T, the law's own x_max from the Chernoff bound at 10⁻⁸
        near = bc.LAWS[c["law"][:-len("/far")]]
        assert c["VT"] == near["VT"] and mp.mpf(bc.LAWS[c["law"]]["x_max"]) > mp.mpf(near["x_max"])
        assert mp.mpf(bc.LAWS[c["law"]]["ladder"][-1][1]) > 1 - mp.mpf(10) ** -8


@pytest.mark.parametrize("law_id", list(bc.LAWS))
def test_phi_is_a_characteristic_function_with_the_laws_moments(law_id):
    """ϕ(0) = 1, ϕ(−a) = conj ϕ(a), |ϕ| <= 1; its first two derivatives at 0 by 50-digit central differences give the
    mean and variance the fixture took from the cumulant function; the stored ladder of F rises from 0 to 1
    (within the 10⁻²⁵ it is computed to)."""
    rec, law = law_by_id(law_id)
    with mp.workdps(50):
        assert abs(law.phi(mp.mpf(0)) - 1) < TEN ** -45
        h = mp.mpf(rec["h"])
        for a in (h / 7, h, 3 * h, 40 * h):
            v = law.phi(a)
            assert abs(v - mp.conj(law.phi(-a))) < TEN ** -45 and abs(v) <= 1
        d = TEN ** -10
        pp, pm = law.phi(d), law.phi(-d)
        mean = mp.im(pp - pm) / (2 * d)
        second = -mp.re(pp - 2 + pm) / (d * d)
        assert abs(mean / mp.mpf(rec["mean"]) - 1) < TEN ** -15
        assert abs((second - mean ** 2) / mp.mpf(rec["variance"]) - 1) < TEN ** -12
        ladder = [(mp.mpf(x), mp.mpf(F)) for x, F in rec["ladder"]]
        tol = TEN ** -25  # what F is computed to: far in the left tail the law's mass is less than that
        assert all(a[0] < b[0] and -tol < a[1] < b[1] + tol and b[1] < 1 for a, b in zip(ladder, ladder[1:]))
        assert sum(b[1] > a[1] + tol for a, b in zip(ladder, ladder[1:])) >= len(ladder) - 3
        assert ladder[-1][1] > 1 - TEN ** -4
    assert rec["halved_step_difference"] <= 1e-20


@pytest.mark.parametrize("law_id,turns", [("h252/q0.5", True), ("q2/q0.001", True), ("q2/q0.999", False), ("short_T/q0.5", False),
                                          ("large_nu_short_T/q0.999", False)])
def test_the_closed_form_angle_is_the_angle_carried_by_continuity(law_id, turns):
    """arg z(γ(a)) of Law.angle against the principal argument unwrapped step by step on a ladder in a fine enough that
    no step turns z by more than 0.2 rad, out to where the series of F ends: they agree everywhere.  z turns
    counter-clockwise (the angle tends to σ·√a·T/2 − π/4); in the laws marked so it has by then crossed the negative real
    axis, where the principal branch of I_ν jumps."""
    rec, law = law_by_id(law_id)
    with mp.workdps(30):
        a_end = mp.mpf(rec["h"]) * rec["terms"]
        carried, a, worst, step = mp.mpf(0), mp.mpf(0), mp.mpf(0), a_end / 4000
        while a < a_end:
            a += step
            turn = mp.arg(law.z(a)) - carried
            turn -= 2 * mp.pi * mp.nint(turn / (2 * mp.pi))
            assert abs(turn) < 0.2
            carried += turn
            worst = max(worst, abs(carried - law.angle(a)))
        assert worst < TEN ** -25 and (carried > mp.pi) == turns


def cir_transform(p, a):
    """E exp(ia·∫₀ᵀV dt) given V0 alone, by the Cox–Ingersoll–Ross (1985) bond-price formula with λ = −ia:
    [2γ e^{(κ+γ)T/2} / ((γ+κ)(e^{γT} − 1) + 2γ)]^{2κθ/σ²} · exp(−V0 · 2λ(e^{γT} − 1) / ((γ+κ)(e^{γT} − 1) + 2γ)),
    the power continued from a = 0 on a ladder of 400 steps"""
    k, th, sg, T, V0 = (mp.mpf(p[n]) for n in ("kappa", "theta", "sigma", "T", "V0"))
    ang = mp.mpf(0)
    for i in range(1, 401):
        lam = -mp.mpc(0, 1) * a * i / 400
        g = mp.sqrt(k * k + 2 * sg * sg * lam)
        den = (g + k) * mp.expm1(g * T) + 2 * g
        base, B = 2 * g * mp.exp((k + g) * T / 2) / den, 2 * lam * mp.expm1(g * T) / den
        turn = mp.arg(base) - ang
        ang += turn - 2 * mp.pi * mp.nint(turn / (2 * mp.pi))
    return mp.exp(2 * k * th / (sg * sg) * mp.mpc(mp.log(abs(base)), ang)) * mp.exp(-B * V0)


@pytest.mark.parametrize("regime,a,leaves_sheet", [("h252", 5, False), ("h252", 900, True), ("nu_63", 500, False)])
def test_phi_mixed_over_the_variance_is_the_cir_transform(regime, a, leaves_sheet):
    """A pin from outside the paper's formula: ∫ ϕ(a | V_T)·p(V_T) dV_T over the non-central χ² density of V_T must be
    the transform of ∫V given V0 alone, which Cox, Ingersoll & Ross give in closed form without a Bessel function.
    At a = 900 of regime h252 (ν = −0.11) z(γ) has crossed the negative real axis: a ϕ on the principal branch of
    I_ν would miss by the factor e^{2πiν}."""
    p = bc.REGIMES[regime]
    with mp.workdps(20):
        k, th, sg, T, V0 = (mp.mpf(p[n]) for n in ("kappa", "theta", "sigma", "T", "V0"))
        em1 = -mp.expm1(-k * T)
        c, d, lam = sg * sg * em1 / (4 * k), 4 * k * th / (sg * sg), 4 * k * mp.exp(-k * T) * V0 / (sg * sg * em1)

        def integrand(v):
            y = v / c
            density = mp.exp(-(y + lam) / 2) * (y / lam) ** (d / 4 - mp.mpf(1) / 2) * mp.besseli(d / 2 - 1, mp.sqrt(lam * y)) / (2 * c)
            return density * bx.Law(p["V0"], v, p["kappa"], p["theta"], p["sigma"], p["T"]).phi(mp.mpf(a))

        m = c * (d + lam)
        mixed = mp.quad(integrand, [0, m / 8, m / 2, m, 2 * m, 4 * m, 10 * m, 40 * m])
        want = cir_transform(p, mp.mpf(a))
        assert abs(mixed - want) < TEN ** -10 * abs(want)
        angle = bx.Law(p["V0"], p["V0"], p["kappa"], p["theta"], p["sigma"], p["T"]).angle(mp.mpf(a))
        assert (angle > mp.pi) == leaves_sheet


@pytest.mark.parametrize("law_id", CHEAP)
def test_the_law_recomputed(law_id):
    """The table behind F rebuilt: the same step and length; the ladder's F to 10⁻²⁵; F(x*) = u to 10⁻²⁰ and the stored
    density at every case of the law; and, in doubles from the same table, ∫(1 − F) and ∫2x(1 − F) give the mean and the
    second moment of the cumulant function (the trapezoid rule on 4000 points up to x_max, beyond which 10⁻⁴·x_max of
    mass at most is left: 10⁻³ relative)."""
    rec, law = law_by_id(law_id)
    with mp.workdps(bx.DPS):
        law.build(mp.mpf(rec["x_max"]))
        assert len(law.table["re"]) == rec["terms"] and abs(law.table["h"] / mp.mpf(rec["h"]) - 1) < TEN ** -30
        for x, F in rec["ladder"]:
            assert abs(law.F(mp.mpf(x)) - mp.mpf(F)) < TEN ** -25
        for c in bc.CASES:
            if c["law"] == law_id:
                x = mp.mpf(c["x"])
                assert abs(law.F(x) - mp.mpf(c["u"])) < TEN ** -20
                assert abs(law.pdf(x) / mp.mpf(c["f"]) - 1) < TEN ** -25
                assert abs(law.pdf(x, 1)) <= c["f1_bound"]
    h, re = law.table_fp64()
    xs = np.linspace(0.0, float(mp.mpf(rec["x_max"])), 4001)
    j = np.arange(1, len(re) + 1)
    F = h * xs / math.pi + 2 / math.pi * (np.sin(np.outer(xs, h * j)) / j) @ re
    assert np.all(np.diff(F) > -1e-12) and abs(F[0]) < 1e-12
    mean, var = float(mp.mpf(rec["mean"])), float(mp.mpf(rec["variance"]))
    assert np.trapezoid(1 - F, xs) == pytest.approx(mean, rel=1e-3)
    assert np.trapezoid(2 * xs * (1 - F), xs) == pytest.approx(var + mean * mean, rel=2e-3)


@pytest.mark.parametrize("law_id", ["short_T/q0.5", "q2/q0.999"])
def test_half_the_step_and_twice_the_cut_off(law_id):
    rec, law = law_by_id(law_id)
    with mp.workdps(bx.DPS):
        law.build(mp.mpf(rec["x_max"]))
        xs = [mp.mpf(c["x"]) for c in bc.CASES if c["law"] == law_id] + [mp.mpf(rec["x_max"])]
        assert law.verify(xs) < TEN ** -20


@functools.lru_cache(maxsize=None)
def _oracle_sample(law_id, u, control, reading):
    case = next(c for c in bc.CASES if c["law"] == law_id and c["u"] == u)
    p, ctl = bc.REGIMES[case["regime"]], bc.CONTROLS[control]
    dist = bk_oracle.LogHestonDistribution(p["S0"], p["V0"], p["kappa"], p["theta"], p["sigma"], p["rho"], p["r"], p["T"])
    trace = []
    x = bk_oracle.sample_from_cf(case["u"], bk_oracle.HestonCFIterator(case["VT"], dist), n=ctl["bk_n_sigma"],
                                 cf_tol=ctl["bk_cf_tol"], atol=ctl["bk_atol"], moment_h=ctl["bk_moment_h"],
                                 maxiter_newton=ctl["bk_newton_maxiter"], maxiter_bisection=ctl["bk_bisect_maxiter"],
                                 trace=trace, root_form=reading[0], bracket_form=reading[1], caps=reading[2])
    return x, trace[0]


def oracle_sample(case, control, reading=(0, 0, 0)):
    """(sample, decision word) of the fp64 oracle; kept, for the tests that ask what the search did"""
    return _oracle_sample(case["law"], case["u"], control, tuple(reading))


def reading_id(reading):
    return "root%d-bracket%d-caps%d" % tuple(reading)


@pytest.fixture(scope="module")
def worst():
    ws = {r: bc.Worst("bk_law_exact (fp64 oracle)" + ("" if r == (0, 0, 0) else ", " + reading_id(r))) for r in bc.READINGS}
    yield ws
    for w in ws.values():
        w.report()


# (reading (0, 0, 0) under the ids it has always had: regime-control)
ORACLE_RUNS = [(regime, control, reading) for reading in bc.READINGS for control in bc.CONTROLS for regime in bc.REGIMES]


@pytest.mark.parametrize("regime,control,reading", ORACLE_RUNS,
                         ids=[f"{g}-{c}" + ("" if r == (0, 0, 0) else "-" + reading_id(r)) for g, c, r in ORACLE_RUNS])
def test_the_fp64_oracle_meets_the_bars(worst, regime, control, reading):
    """oracle/bk_oracle.py's sample for every case's (V_T, u) under the case's controls, in every reading of the root
    search, held to the exact law at the device test's bar (the recovery term left out: the oracle hands over ∫V
    itself).  A far case's sample must besides lie inside `reach` (Worst.check fails it otherwise) and must not be
    max_guess: the condition the fixture's maker chose their uniforms under."""
    bad = []
    for case in bc.cases_of(regime):
        x, decision = oracle_sample(case, control, reading)
        bad.append(worst[reading].check(case, control, mp.mpf(x), decision, "oracle"))
        if bc.is_far(case) and bc.branch_of(decision) == bc.DEC_MAXGUESS:
            bad.append(f"{control} {case['law']} u={case['u']:g}: left by the max_guess exit")
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("reading", bc.READINGS, ids=reading_id)
@pytest.mark.parametrize("control", list(bc.CONTROLS))
def test_every_reading_reaches_the_ladder(control, reading):
    """Conditions on the INPUTS, not measurements: the fixture sends the oracle down the fall-back ladder (branch 1) in
    every reading, under either control set, on at least 5 of the 84 original cases, and under the tight set on every
    far case with the low uniform (10⁻⁶, or the 10⁻⁵ it was moved to); the bit-pattern bisection (bracket_form 1) then runs to adjacent floats, 40 halvings at the
    very least.  If a change of the fixture breaks one of these, the fixture is what has to change."""
    ladders = {}
    for case in bc.CASES:
        decision = oracle_sample(case, control, reading)[1]
        if bc.branch_of(decision) == bc.DEC_BISECT:
            ladders[(case["law"], case["u"])] = bc.iterations_of(decision)
    assert sum(not law.endswith("/far") for law, _ in ladders) >= 5, ladders
    if control == "tight":
        assert all((c["law"], c["u"]) in ladders for c in bc.FAR_LOW), ladders
    if reading[1] == 1:
        assert min(ladders.values()) >= 40, ladders
