"""Broadie–Kaya samples of the device against the EXACT conditional law of ∫V given (V0, V_T) (oracle/bk_law_exact.py at
40-50 digits, written from the paper; tests/golden/bk_law_exact.json): if the kernels return x for the uniform u, then
|F(x) − u| must be within the bar of tests/bk_law_exact_cases.py — stop + E_alg + 20·max(e64, ε·A) — whatever way the
root search went.  No decision has to match anything: the decision word only says which stopping rule applies.

The cases are fed through HH_NOISE_REPLAY as [V_T | u | Z] with Z = 0, so that log S_T is affine in ∫V and the sample
is recovered from the returned spot in mpmath (bk_law_exact_cases.integral_from_spot).  Every case of the nine regimes
and the absorbed variance, under the shipped controls and under tight ones (atol = cf_tol = 10⁻¹⁰, n_σ = 12: the CF,
the series and the search pinned to ~nine digits of the CDF), as
  (a) one solve of 700 trajectories (three tiles, the last ragged), the cases 67 lanes apart among filler trajectories,
  (b) one solve per case,
both with the default term cache and with HH_OPT_BK_TERM_CACHE = 8, where every trajectory runs whole in the fall-back
kernel; and (c) through hh_mc_solve_multi with a bumped spot, where bk_refinish_kernel finishes the second model from
the ∫V the chain kept.  The module prints its worst residual/bar per regime and control set at its end (`-s`)."""
import ctypes as C

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import bk_law_exact_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu

N, STRIDE, FIRST = 700, 67, 5   # 700 = 2·256 + 188; 67 is prime to 700: case i sits in lane (5 + 67·i) mod 700
BUMP = 1.001


@pytest.fixture(scope="module")
def worst():
    w = bc.Worst("bk_law_exact (device)")
    yield w
    w.report()


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def config_of(control, draws, reading=(0, 0, 0)):
    """`reading`: (bk_root_form, bk_bracket_form, bk_caps) — tests/test_gpu_bk_law_exact_forms.py runs the other seven"""
    n = draws.shape[1]
    c = _ffi.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, noise_mode=_ffi.HH_NOISE_REPLAY, replay=draws.ravel())
    for k, v in bc.CONTROLS[control].items():
        setattr(c, k, type(getattr(c, k))(v))
    c.bk_root_form, c.bk_bracket_form, c.bk_caps = reading
    return c


def draws_of(cases, n, positions, seed):
    """[V_T | u | Z = 0]: the cases at `positions`, everywhere else a case's V_T (in turn) with a uniform of its own"""
    rng = np.random.default_rng(seed)
    d = np.zeros((3, n))
    d[0] = [cases[i % len(cases)]["VT"] for i in range(n)]
    d[1] = rng.uniform(0.02, 0.98, size=n)
    for c, at in zip(cases, positions):
        d[0, at], d[1, at] = c["VT"], c["u"]
    return np.ascontiguousarray(d)


def solve(ctx, regime, control, draws, S0=None, reading=(0, 0, 0)):
    p = dict(bc.REGIMES[regime])
    if S0 is not None:
        p["S0"] = S0
    m = _ffi.make_model(**p)
    c = config_of(control, draws, reading)
    n = draws.shape[1]
    res, term = _ffi.hh_result(), np.zeros(n)
    ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(m), C.byref(c), C.byref(res), term.ctypes.data))
    dec = np.zeros(n, dtype=np.uint32)
    ctx.check(ctx.lib.hh_bk_decisions(ctx.handle, n, dec.ctypes.data, None))
    assert res.n_paths_done == n and np.all(np.isfinite(term)) and np.all(term > 0)
    return term, dec, m, c


def check(worst, cases, control, term, dec, positions, where, S0=None):
    bad = []
    for c, at in zip(cases, positions):
        x = bc.integral_from_spot(c, term[at], S0)
        bad.append(worst.check(c, control, x, dec[at], f"{where} lane {at}", A=bc.recovery_allowance(c, S0)))
    return [b for b in bad if b]


def with_cache(ctx, cache):
    ctx.set_option(_ffi.HH_OPT_BK_TERM_CACHE, cache)


@pytest.mark.parametrize("cache", [256, 8])
@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
def test_cases_among_filler_trajectories(ctx, worst, regime, control, cache):
    cases = bc.cases_of(regime)
    positions = [(FIRST + STRIDE * i) % N for i in range(len(cases))]
    assert len(set(p // 64 for p in positions)) >= min(len(cases), 9) and N % 256
    draws = draws_of(cases, N, positions, seed=len(regime))
    with_cache(ctx, cache)
    try:
        term, dec, _, _ = solve(ctx, regime, control, draws)
    finally:
        with_cache(ctx, 256)
    if cache == 8:  # (a series has its first term at least; longer than the cache: the fall-back kernel)
        assert np.all((dec[positions] >> 31) == 1)
    bad = check(worst, cases, control, term, dec, positions, f"n={N} cache={cache}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cache", [256, 8])
@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
def test_one_case_per_solve(ctx, worst, regime, control, cache):
    bad = []
    with_cache(ctx, cache)
    try:
        for c in bc.cases_of(regime):
            term, dec, _, _ = solve(ctx, regime, control, draws_of([c], 1, [0], seed=0))
            bad += check(worst, [c], control, term, dec, [0], f"n=1 cache={cache}")
    finally:
        with_cache(ctx, 256)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("control", list(bc.CONTROLS))
@pytest.mark.parametrize("regime", list(bc.REGIMES))
def test_second_model_finished_from_the_kept_integral(ctx, worst, regime, control):
    """hh_mc_solve_multi, two models that differ in the spot: the first runs the chain, bk_refinish_kernel finishes the
    second from the ∫V the chain kept.  Model 0's spots are hh_mc_solve's bit for bit, so the decision words of that
    solve describe the chain; model 1's samples are recovered with ITS spot and held to the same law."""
    cases = bc.cases_of(regime)
    n = 333
    positions = [(FIRST + 29 * i) % n for i in range(len(cases))]
    draws = draws_of(cases, n, positions, seed=1 + len(regime))
    term, dec, m0, c = solve(ctx, regime, control, draws)
    S1 = bc.REGIMES[regime]["S0"] * BUMP
    m1 = _ffi.make_model(**dict(bc.REGIMES[regime], S0=S1))
    terms = [np.zeros(n), np.zeros(n)]
    res = (_ffi.hh_result * 2)()
    ptrs = (C.c_void_p * 2)(terms[0].ctypes.data, terms[1].ctypes.data)
    ctx.check(ctx.lib.hh_mc_solve_multi(ctx.handle, (_ffi.hh_model * 2)(m0, m1), 2, C.byref(c), res, ptrs))
    np.testing.assert_array_equal(terms[0], term)
    bad = check(worst, cases, control, terms[1], dec, positions, "second model", S0=S1)
    assert not bad, "\n".join(bad)
