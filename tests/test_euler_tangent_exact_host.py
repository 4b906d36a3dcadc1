"""The Euler-tangent reference (oracle/euler_exact.py: the scheme with its step-by-step dual rules in mpmath at 50
digits) on the committed cases (tests/golden/euler_tangent_exact.json), and the C oracle (oracle/hh_oracle.c) held to
it PER PATH at the bars of tests/euler_tangent_cases.py: S_T, the price contribution and all eight partials of every
usable path of every case — the clip (FV, V0zero, allzero), the classic step form, κ·dt > 1 (kdt) among them.  This
is the first pin of the oracle's dual rules that does not come from the hand that wrote them.  The module prints its
worst error/bar per kind of comparison at its end (`-s`).

Worst error/bar when this was written: 0.079 per path (∂/∂S0, FV-s16-split-anti), 0.050 on a sum.

One condition of the cases is waived where it cannot hold: allzero-split is a split-form clip case, but its v and K_v are
exact zeros at every step, so [v > 0] ≠ [K_v > 0] never occurs there (`flags_differ` is false for it)."""
import os

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from oracle import euler_exact as ex  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests.euler_tangent_cases import BY_ID, IDS, NS, SLOTS  # noqa: E402


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("euler_tangent_exact (C oracle)")
    yield w
    w.report()


def _oracle_solve(oracle, case, strike, cp, paths):
    m = etc.model_of(case, strike, cp)
    c = etc.config_of(case, paths, path_major=True)
    res, term, _ = oracle.mc_solve(m, c, n_threads=1)
    return res, term


def test_the_file_is_small_and_complete():
    assert os.path.getsize(etc.GOLDEN) < 100_000
    tags = {c["tag"] for c in etc.CASES}
    assert tags == {"H252", "Q2", "FV", "kdt", "V0zero", "allzero", "GBM"}
    for tag in tags - {"GBM"}:
        assert {c["em_split"] for c in etc.CASES if c["tag"] == tag} == {0, 1}
    for tag in ("H252", "FV", "kdt"):
        assert {c["antithetic"] for c in etc.CASES if c["tag"] == tag} == {0, 1}
    assert {c["n_steps"] for c in etc.CASES if c["tag"] == "H252"} >= {1, 2, 7, 16, 50}
    for c in etc.CASES:
        assert sorted(c["payoff_list"]) == sorted([(c["S0"], 1.0), (c["S0"] / 2, 1.0), (3 * c["S0"], 1.0), (c["S0"], -1.0)])
        assert np.array_equal(c["dW"] * 4096, np.rint(c["dW"] * 4096))  # multiples of 2^-12: exact doubles everywhere


@pytest.mark.parametrize("name", IDS)
def test_digest_and_generator_conditions(name):
    """The reference module still computes what it computed when the cases were written (30 digits of the 50-digit sum
    over the usable paths, per payoff and slot), and the cases still exercise what they are there for."""
    case = BY_ID[name]
    ref = etc.reference(case)
    for j, pj in enumerate(ref["payoffs"]):
        assert (~pj["usable"]).sum() <= etc.MAX_UNUSABLE * ref["n"], (name, j)
        paths = [i for i in range(ref["n"]) if pj["usable"][i]]
        with mp.workdps(ex.DPS):
            got = [mp.nstr(mp.fsum(pj["price"][i][s] for i in paths), 30) for s in range(1 + NS)]
        assert got == case["digests"][j], (name, j)
    if case["clip"]:
        assert ref["clip_fraction"] >= etc.MIN_CLIP_FRACTION
    if case["flags_differ"]:
        assert case["em_split"] and ref["pos_ne_wpos"] >= 1
    if case["tag"] == "kdt":
        assert case["kappa"] * case["T"] / case["n_steps"] > 1.0


@pytest.mark.parametrize("name", IDS)
def test_fp64_restatement_stays_near_the_reference(name):
    """What sizes the bars from below: the fp64 run of the same formulas stays within 1e-11·|value| of the 50-digit run
    on every usable path, payoff and slot (measured: at most 7e-13), and within 1e-13·S_T on every terminal."""
    ref = etc.reference(BY_ID[name])
    for pj in ref["payoffs"]:
        u = np.flatnonzero(pj["usable"])
        vals = np.array([[abs(float(t)) for t in row] for row in pj["price"]])[u]
        assert np.all(pj["price_e64"][u] <= 1e-11 * vals)
    assert np.all(ref["S_e64"] <= 1e-13 * np.array([[float(t) for t in row] for row in ref["S"]]))


@pytest.mark.parametrize("name", IDS)
def test_bars_are_fp64_sized(name):
    """The bars against the VALUES they guard, so that a magnitude A that outgrew its value cannot hollow them out.
    Per usable path, payoff and slot with a nonzero value:
      * the bar's median over a case is at most 1e-11·|value| (measured: 1e-14 … 5e-12), and at least 95 % of a case's
        bars are below 1e-9·|value|, the tightest bar the accumulated Greeks are held to elsewhere;
      * every bar, those of zero values too, is below LIMIT·max(|value|, the slot's median nonzero |value| over the
        case's paths).  A partial that cancelled to a fraction of its slot's usual size, or to an exact zero, keeps the
        bar of its terms, hence the max; a slot that is zero on every path (∂/∂κ after one step from V0 = θ) is held
        against the price's median instead.
    Per payoff and slot, the sum bar is below LIMIT·Σ|terms|, and below LIMIT·|sum| where the paths did not cancel to
    under a tenth of Σ|terms| (an all-zero slot: against the same median as above).
    LIMIT is 1e-9 up to 16 steps and 1e-8 at 50: A is a worst-case first-order bound, which lets the error of the
    variance grow by 1 + σ|dW|/(2√v) per step where a real rounding error grows like a random walk.  Measured on
    H252-s50-split: 12 of 288 bars above 1e-9·|value|, the largest 3.4e-8 (4.4e-9 of its slot's median); sum bars up
    to 1.1e-9·Σ|terms|.  Every other case: at most 1.9e-10 and 8.5e-11.
    S_T: every bar below 1e-10·S_T (measured: at most 2.3e-11, at 50 steps)."""
    case = BY_ID[name]
    etc.assert_bars_are_fp64_sized(etc.reference(case), int(case["antithetic"]), 1e-9 if case["n_steps"] <= 16 else 1e-8)


@pytest.mark.parametrize("name", IDS)
def test_c_oracle_path_by_path(oracle, worst, name):
    """hho_mc_solve as REPLAY with n_paths = 1, eight unit seeds: dprice[k] is the path's discounted partial."""
    case = BY_ID[name]
    ref = etc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        for i in np.flatnonzero(ref["payoffs"][j]["usable"]):
            res, term = _oracle_solve(oracle, case, strike, cp, [int(i)])
            bad += etc.check_solve(worst, case, ref, j, [int(i)], res, term, "oracle")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", IDS)
def test_c_oracle_all_paths_in_one_call(oracle, worst, name):
    case = BY_ID[name]
    ref = etc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        paths = [int(i) for i in np.flatnonzero(ref["payoffs"][j]["usable"])]
        res, term = _oracle_solve(oracle, case, strike, cp, paths)
        assert res.n_paths_done == len(paths)
        bad += etc.check_solve(worst, case, ref, j, paths, res, term, "oracle")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", [n for n in IDS if BY_ID[n]["tag"] == "allzero"])
def test_the_convention_at_the_clip(oracle, name):
    """V0 = 0, θ = 0: the variance is an exact zero at every step, so the √'s tangent is taken at the clip throughout —
    0 by the convention of DESIGN.md §2.  Then nothing reaches x from V0, κ, θ or σ: those partials are exact zeros,
    S_T = S0·e^{rT}, and ∂price/∂S0 = disc·e^{rT}·[itm]·cp."""
    case = BY_ID[name]
    ref = etc.reference(case)
    assert ref["clip_fraction"] == 1.0
    with mp.workdps(ex.DPS):
        growth = mp.exp(mp.mpf(case["r_drift"]) * mp.mpf(case["T"]))
        ST = mp.mpf(case["S0"]) * growth
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        pj = ref["payoffs"][j]
        assert pj["usable"].all()
        itm = 1.0 if cp * (float(ST) - strike) > 0 else 0.0
        bars = etc.path_bar(pj["price_e64"], pj["price_A"])
        sbar = etc.path_bar(ref["S_e64"], ref["S_A"])
        for i in range(ref["n"]):
            res, term = _oracle_solve(oracle, case, strike, cp, [i])
            for who, dprice in (("reference", [float(t) for t in pj["price"][i][1:]]), ("oracle", list(res.dprice))):
                for slot in ("V0", "kappa", "theta", "sigma"):
                    assert dprice[SLOTS.index(slot)] == 0.0, (who, slot, i)
                with mp.workdps(ex.DPS):
                    want = mp.mpf(case["discount"]) * growth * itm * cp
                assert etc.err(dprice[0], want) <= bars[i][1], (who, i)
            assert etc.err(term[0], ST) <= sbar[0][i]
            assert etc.err(float(ref["S"][0][i]), ST) <= sbar[0][i]
