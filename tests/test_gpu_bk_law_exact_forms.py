"""The seven other readings of the reference's two `find_zero` calls (hh_config.bk_root_form / bk_bracket_form /
bk_caps other than 0, 0, 0: every trajectory runs whole in tail_whole_trajectory, csrc/hh_bk.hip — Order2's Steffensen
probe and guarded secant step with its two convergence rules, the bisection over the bit patterns of the ends, Roots'
own caps) held to the EXACT conditional law of ∫V, at the bar of tests/bk_law_exact_cases.py and with the machinery of
tests/test_gpu_bk_law_exact.py, which does this for reading (0, 0, 0).  No decision has to match anything; the decision
word only says which stopping rule the bar takes.  What tests/test_gpu_bk_root_forms.py cannot see at its 3e-5 — an
Order2 iterate accepted that should have been rejected, a bit-pattern bisection ended a few dozen halvings early, a
bracket kept on the wrong side — moves |F(x) − u| by orders more than the bar under the tight controls.

  (a) every regime's cases (the far ones with them) among filler trajectories in one solve of 700, both control sets,
      with the term cache at 256 and at 8;
  (b) reading (1, 1, 1), the one ADVICE.md takes for the reference's: one solve per case, a single trajectory in the
      tail kernel's 64-workgroup launch;
  (c) readings (1, 1, 1) and (0, 1, 0): a second model finished by bk_refinish_kernel from the ∫V the chain kept;
  (d) the ladder is reached on the device, and runs as long as the reading says;
  (e) a reading changes only what it names.
The solves of (a) at cache 256 are kept and serve (d) and (e).  The module prints its worst residual/bar per reading,
regime and control set at its end (`-s`)."""
import ctypes as C

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import bk_law_exact_cases as bc  # noqa: E402
from tests.test_gpu_bk_law_exact import BUMP, FIRST, N, STRIDE, check, ctx, draws_of, solve, with_cache  # noqa: E402,F401

pytestmark = pytest.mark.gpu

FORMS = [r for r in bc.READINGS if r != (0, 0, 0)]
ROOTS_MAXITERS = 40   # Roots.jl's own `maxiters` of a secant-type method: what caps = 1 puts in place of bk_newton_maxiter


def form_id(reading):
    return "root%d-bracket%d-caps%d" % tuple(reading)


@pytest.fixture(scope="module")
def worst():
    ws = {r: bc.Worst(f"bk_law_exact (device), {form_id(r)}") for r in FORMS}
    yield ws
    for w in ws.values():
        w.report()


def positions_of(cases, n=N, stride=STRIDE):
    return [(FIRST + stride * i) % n for i in range(len(cases))]


_SOLVED = {}


def solved(ctx, reading, regime, control, cache=256):
    """(spots, decision words) of the n = 700 solve of (a): computed once, left unchanged"""
    key = (reading, regime, control, cache)
    if key not in _SOLVED:
        cases = bc.cases_of(regime)
        draws = draws_of(cases, N, positions_of(cases), seed=len(regime))
        with_cache(ctx, cache)
        try:
            term, dec, _, _ = solve(ctx, regime, control, draws, reading=reading)
        finally:
            with_cache(ctx, 256)
        term.setflags(write=False)
        dec.setflags(write=False)
        _SOLVED[key] = (term, dec)
    return _SOLVED[key]


@pytest.mark.parametrize("cache", [256, 8])
@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
@pytest.mark.parametrize("reading", FORMS, ids=form_id)
def test_cases_among_filler_trajectories(ctx, worst, reading, regime, control, cache):
    cases = bc.cases_of(regime)
    positions = positions_of(cases)
    assert len(set(p // 64 for p in positions)) >= min(len(cases), 9) and N % 256
    term, dec = solved(ctx, reading, regime, control, cache)
    # Bit 31 says "the series outgrew the term cache, so the trajectory ran whole in the fall-back kernel".  Under a
    # reading other than (0, 0, 0) EVERY trajectory runs there whatever its series' length, and tail_whole_trajectory
    # starts the word from 0: the bit is clear at either cache size, and tells nothing.
    assert np.all((dec >> 31) == 0)
    bad = check(worst[reading], cases, control, term, dec, positions, f"n={N} cache={cache}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
def test_one_case_per_solve(ctx, worst, regime, control):
    reading, bad = (1, 1, 1), []
    for c in bc.cases_of(regime):
        term, dec, _, _ = solve(ctx, regime, control, draws_of([c], 1, [0], seed=0), reading=reading)
        bad += check(worst[reading], [c], control, term, dec, [0], "n=1")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
@pytest.mark.parametrize("reading", [(1, 1, 1), (0, 1, 0)], ids=form_id)
def test_second_model_finished_from_the_kept_integral(ctx, worst, reading, regime, control):
    """hh_mc_solve_multi, two models that differ in the spot: the first runs the chain (here: the tail kernel, every
    trajectory), bk_refinish_kernel finishes the second from the ∫V it kept.  Model 0's spots are hh_mc_solve's bit for
    bit; model 1's samples are recovered with ITS spot and held to the same law."""
    cases = bc.cases_of(regime)
    n = 333
    positions = positions_of(cases, n, 29)
    draws = draws_of(cases, n, positions, seed=1 + len(regime))
    term, dec, m0, c = solve(ctx, regime, control, draws, reading=reading)
    S1 = bc.REGIMES[regime]["S0"] * BUMP
    m1 = _ffi.make_model(**dict(bc.REGIMES[regime], S0=S1))
    terms = [np.zeros(n), np.zeros(n)]
    res = (_ffi.hh_result * 2)()
    ptrs = (C.c_void_p * 2)(terms[0].ctypes.data, terms[1].ctypes.data)
    ctx.check(ctx.lib.hh_mc_solve_multi(ctx.handle, (_ffi.hh_model * 2)(m0, m1), 2, C.byref(c), res, ptrs))
    np.testing.assert_array_equal(terms[0], term)
    bad = check(worst[reading], cases, control, terms[1], dec, positions, "second model", S0=S1)
    assert not bad, "\n".join(bad)


def branch(dec):
    return (np.asarray(dec) >> bc.DEC_BRANCH_SHIFT) & 3


def iterations(dec):
    return (np.asarray(dec) >> bc.DEC_ITERS_SHIFT) & 0xff


@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("reading", FORMS, ids=form_id)
def test_the_ladder_is_reached_on_the_device(ctx, reading, control):
    """The fp64 oracle takes the fall-back ladder on 5 or more of the 84 original cases in every reading and control
    set, and under the tight set on every far case with the low uniform (tests/test_bk_law_exact_host.py).  The device
    may decide two cases otherwise — tests/test_gpu_bk.py's allowance for flipped decisions, max(2, 1 %) — so: at least
    3, and every one of those far cases, whose uniform is far below anything the first search accepts.  The bit-pattern
    bisection ran to adjacent floats (40 halvings at the very least; ~62 from (0, max_guess)) on EVERY trajectory of
    the solves that took it; and with the caps as written, no bisection ran past bk_bisect_maxiter."""
    ladders, far_low = 0, []
    for regime in bc.REGIMES:
        cases = bc.cases_of(regime)
        _, dec = solved(ctx, reading, regime, control)
        at = dict(zip(((c["law"], c["u"]) for c in cases), positions_of(cases)))
        ladders += sum(branch(dec[at[c["law"], c["u"]]]) == bc.DEC_BISECT for c in cases if not bc.is_far(c))
        far_low += [(c["law"], int(dec[at[c["law"], c["u"]]])) for c in cases if bc.is_far(c) and c["u"] < 0.5]
        ran = iterations(dec)[branch(dec) == bc.DEC_BISECT]
        if reading[1] == 1 and ran.size:
            assert ran.min() >= 40, (regime, int(ran.min()))
        if reading[2] == 0 and control == "shipped" and ran.size:
            assert ran.max() <= bc.CONTROLS[control]["bk_bisect_maxiter"], (regime, int(ran.max()))
    print(f"\nbk_law_exact (device), {form_id(reading)} {control}: {ladders} of the 84 original cases took the ladder")
    assert ladders >= 3
    assert len(far_low) == len(bc.FAR_LOW) == 3
    if control == "tight":
        assert all(bc.branch_of(d) == bc.DEC_BISECT for _, d in far_low), [(law, hex(d)) for law, d in far_low]


def first_search_cap(control):
    """the smaller of the two caps a pair of readings that differ in bk_caps puts on the first search, in EVALUATIONS:
    the secant counts evaluations (two before its first step), Order2 steps of one or two evaluations each — a search
    with fewer evaluations than this met neither cap"""
    return min(bc.CONTROLS[control]["bk_newton_maxiter"], ROOTS_MAXITERS)


@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
def test_a_reading_changes_only_what_it_names(ctx, regime, control):
    """All 700 trajectories of the solves of (a), among the seven readings of this module ((0, 0, 0) runs on the fast
    chain, other code).  Where the first search was accepted (branch 0) no bisection ran: bk_bracket_form cannot have
    mattered, and the decision word and the spot are the same bits with either.  Where it was accepted after fewer
    evaluations than the smaller cap, bk_caps cannot have mattered."""
    got = {r: solved(ctx, r, regime, control) for r in FORMS}
    pairs = 0
    print(f"\nbk_law_exact (device), {regime} {control}: first search accepted on "
          f"{[int((branch(got[r][1]) == 0).sum()) for r in FORMS]} of {N} trajectories, readings {FORMS}")
    for rf, cp in ((0, 1), (1, 0), (1, 1)):
        (t0, d0), (t1, d1) = got[rf, 0, cp], got[rf, 1, cp]
        sel = branch(d0) == 0
        assert sel.any()
        assert np.array_equal(d0[sel], d1[sel]) and t0[sel].tobytes() == t1[sel].tobytes(), (rf, cp)
        pairs += 1
    for rf, bf in ((0, 1), (1, 0), (1, 1)):
        (t0, d0), (t1, d1) = got[rf, bf, 0], got[rf, bf, 1]
        sel = (branch(d0) == 0) & ((d0 & 0xff) < first_search_cap(control))
        assert sel.any()
        assert np.array_equal(d0[sel], d1[sel]) and t0[sel].tobytes() == t1[sel].tobytes(), (rf, bf)
        pairs += 1
    assert pairs == 6
