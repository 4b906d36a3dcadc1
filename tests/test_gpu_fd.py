"""Crank–Nicolson grids on the device (hh_fd_solve, csrc/hh_fd.hip): price, delta and gamma against the 50-digit run of
the serial restatement (tests/fd_cases.py, tests/golden/fd_exact.json) inside bars that come from the restatement's own
fp64 error, over every kernel form and both sides of every layout boundary; baskets against single solves bit for
bit; `solve`, the basket and finite-difference Greeks; the orderings American exercise implies."""
import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from hedgehog_jl_amd.pde import FDInputs, fd_device
from tests import fd_cases as fc

pytestmark = pytest.mark.gpu

REF = hh.Date(2020, 1, 1)
GOLD = fc.load_golden()
RUNS = fc.run_list()
GROUPS = sorted({(r[3], r[4], r[5]) for r in RUNS})


def inputs_of(rows):
    """FDInputs from rows of fc.scalars(...)"""
    a = np.array([r[:7] for r in rows], dtype=np.float64)
    return FDInputs(*(np.ascontiguousarray(a[:, k]) for k in range(7)), np.array([r[7] for r in rows], dtype=np.int32))


def device(rows, M, N, R):
    return np.stack(fd_device(inputs_of(rows), M, N, R), axis=1)   # [n][price, delta, gamma]


_results = {}


def device_runs(M, N, R):
    """every run of one (M, N, R) in one launch, once per process"""
    if (M, N, R) not in _results:
        runs = [r for r in RUNS if (r[3], r[4], r[5]) == (M, N, R)]
        _results[(M, N, R)] = (runs, device([fc.scalars(r) for r in runs], M, N, R))
    return _results[(M, N, R)]


@pytest.mark.parametrize("M,N,R", GROUPS)
def test_price_delta_gamma_against_the_50_digit_run(M, N, R):
    runs, got = device_runs(M, N, R)
    worst = 0.0
    for run, row in zip(runs, got):
        exact, e64 = GOLD[run]
        bar = fc.bars(run, e64)
        miss = np.array([fc.err(row[k], exact[k]) for k in range(3)])
        worst = max(worst, float(np.max(miss / bar)))
        print(f"\n{run}: device {row.tolist()} |diff| {miss.tolist()} bar {bar.tolist()} e64 {e64}")
        assert np.all(miss <= bar), (run, miss.tolist(), bar.tolist())
    print(f"(M, N, R) = {(M, N, R)}: worst |diff| / bar = {worst:.3f}")


def test_the_runs_cover_the_layout_and_the_phases():
    Ms = {r[3] for r in RUNS}
    assert Ms >= {4, 8, 62, 64, 66, 128, 130, 200}
    for top in (64, 128, 256, 512, _ffi.HH_FD_FORM_A_MAX_SPACE, 2048):   # a form's largest M, and the next form's first
        assert {top, top + 2} <= Ms, top
    assert _ffi.HH_FD_MAX_SPACE in Ms
    for M in fc.M_SMALL:
        assert {(r[4], r[5]) for r in RUNS if r[3] == M and r[6] == 6.0} >= set(fc.NR_ALL)
    assert {r[4] for r in RUNS} == {1, 2, 3, 50} and {0, 2} <= {r[5] for r in RUNS}
    assert all(((ci, cp, st, 200, 50, 2, 6.0) in GOLD) for ci in range(len(fc.CASES)) for cp, st in fc.SIDES)
    assert set(RUNS) == set(GOLD)


def mixed_rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        S0, K, r, sigma, T = fc.CASES[k % len(fc.CASES)]
        K = float(K * rng.uniform(0.8, 1.25))
        T = float(T * rng.choice([0.5, 1.0, 1.5]))
        cp, style = fc.SIDES[int(rng.integers(4))]
        rows.append((S0, K, cp, sigma, r, T, fc.half_width(S0, K, r, sigma, T), style))
    return rows


@pytest.mark.parametrize("M,N,R", [(66, 7, 2), (200, 5, 1), (1026, 3, 2)])
def test_a_basket_equals_single_solves_bit_for_bit(M, N, R):
    """1, 3, 65 and 1025 options with mixed styles, sides and expiries, in permuted order: the same bits as alone"""
    rows = mixed_rows(1025 if M < 1000 else 65, 11)
    full = device(rows, M, N, R)
    singles = {k: device([rows[k]], M, N, R)[0] for k in (0, 1, 2, 64, len(rows) - 1)}
    for k, one in singles.items():
        assert one.tobytes() == full[k].tobytes(), k
    perm = np.random.default_rng(5).permutation(len(rows))
    for n in (1, 3, 65, len(rows)):
        idx = perm[:n]
        got = device([rows[i] for i in idx], M, N, R)
        assert got.tobytes() == full[idx].tobytes(), n
    assert device(rows, M, N, R).tobytes() == full.tobytes()   # two calls, the same bits
    assert np.all(np.isfinite(full))


def test_null_greek_outputs(hhlib):
    rows = mixed_rows(5, 3)
    inp = inputs_of(rows)
    want = device(rows, 130, 9, 2)
    for skip in ((), ("delta",), ("gamma",), ("delta", "gamma")):
        out = {k: np.full(5, -7.0) for k in ("price", "delta", "gamma")}
        ptr = lambda k: None if k in skip else out[k].ctypes.data  # noqa: E731
        rc = hhlib.lib.hh_fd_solve(hhlib.handle, 130, 9, 2, 5, inp.spots.ctypes.data, inp.strikes.ctypes.data,
                                   inp.cps.ctypes.data, inp.sigmas.ctypes.data, inp.rates.ctypes.data,
                                   inp.expiries.ctypes.data, inp.half_widths.ctypes.data, inp.styles.ctypes.data,
                                   out["price"].ctypes.data, ptr("delta"), ptr("gamma"))
        assert rc == _ffi.HH_OK
        for j, k in enumerate(("price", "delta", "gamma")):
            assert np.array_equal(out[k], np.full(5, -7.0) if k in skip else want[:, j]), (skip, k)


def test_solve_the_basket_and_fd_greeks():
    """`solve` prices what fd_inputs states; a basket is its single solves; European Spot == Forward; a bumped-spot
    central difference of the price lies near the grid's delta.  Bound on the two deltas' distance, on the (512, 256)
    grid with a relative bump of 1e-2 (the spot moves by ±1): each bumped price carries the grid's own error, at most
    E = 1.5e-3 there (the bounds tests/test_fd_host.py holds the scheme to, against the closed form and the tree), so
    the difference quotient moves by at most 2E / 2 = 1.5e-3; the bump's own truncation is (ΔS)²·|∂³V/∂S³|/6 with
    |∂³V/∂S³| <= 1e-3 here (Γ = 0.019, ∂Γ/∂S = −Γ·(d1/(σ√T) + 1)/S), below 2e-4; the grid delta's O(h²) error is
    smaller still.  2e-3 in all."""
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    expiry = hh.Date(2021, 1, 1)
    meth = hh.CrankNicolsonMethod(256, 128)
    payoffs = [hh.VanillaOption(K, expiry, ex, cp, hh.Spot()) for K in (90.0, 100.0) for ex in (hh.European(), hh.American())
               for cp in (hh.Call(), hh.Put())]
    payoffs.append(hh.VanillaOption(100.0, expiry, hh.European(), hh.Put(), hh.Forward()))
    basket = hh.solve(hh.BasketPricingProblem(payoffs, m), meth)
    for p, s in zip(payoffs, basket.solutions):
        one = hh.solve(hh.PricingProblem(p, m), meth)
        assert isinstance(one, hh.PDESolution) and (one.price, one.delta, one.gamma) == (s.price, s.delta, s.gamma)
        inp = hh.fd_inputs([p], m, meth)
        row = (inp.spots[0], inp.strikes[0], inp.cps[0], inp.sigmas[0], inp.rates[0], inp.expiries[0], inp.half_widths[0],
               int(inp.styles[0]))
        want = fc.restate(fc.FP64, *row, 256, 128, 2)
        assert one.price == pytest.approx(want[0], abs=1e-9) and one.delta == pytest.approx(want[1], abs=1e-9)
    assert basket.solutions[-1].price == basket.solutions[5].price   # European put at 100: Forward() == Spot()
    for p in (payoffs[5], payoffs[7]):   # the European and the American put at 100
        prob = hh.PricingProblem(p, m)
        fine = hh.CrankNicolsonMethod(512, 256)
        fd = hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.FiniteDifference(1e-2, hh.FDCentral()), fine).greek
        grid = hh.solve(prob, fine).delta
        print(f"\nFD delta {fd!r}, grid delta {grid!r}")
        assert abs(fd - grid) <= 2e-3 and -1.0 < grid < 0.0


def test_orderings_of_american_exercise():
    """On the committed runs.  The American call is the European call within the two bars wherever the rate is positive:
    there the continuation exceeds the intrinsic value by at least K·(1 − e^{−rτ}) > 0, far above the scheme's error, and
    the max never binds.  At r = 0 (the last case) that margin is the put's value, which vanishes deep in the money, below
    the scheme's truncation error: the max binds at some nodes in exact arithmetic too — the 50-digit runs differ by
    2.2e-7 at (200, 50, 2) and by up to 6.9e-7 over the committed runs — so there the device's difference is held to the
    50-digit difference instead, and to being non-negative.  An American put is worth at least the European put (the
    max only raises values, and the matrices' inverses are positive — less the two bars) and at least its intrinsic value
    (the spot is a node: V_c = max(·, g_c) at every step; g_c is K − exp(ln S0), the intrinsic value to a rounding of
    S0 — one bar)."""
    for M, N, R in ((200, 50, 2), (64, 50, 2), (1026, 50, 2)):
        runs, got = device_runs(M, N, R)
        by = {r: row for r, row in zip(runs, got)}
        for r in runs:
            ci, cp, style, _, _, _, n_std = r
            if style != fc.AMERICAN:
                continue
            eu = (ci, cp, fc.EUROPEAN, M, N, R, n_std)
            slack = fc.bars(r, GOLD[r][1])[0] + fc.bars(eu, GOLD[eu][1])[0]
            S0, K, rate = fc.CASES[ci][:3]
            if cp > 0:
                exact = float(GOLD[r][0][0] - GOLD[eu][0][0])
                print(f"\n{r}: American − European call {by[r][0] - by[eu][0]:.3e} (50 digits: {exact:.3e}), slack {slack:.3e}")
                assert abs((by[r][0] - by[eu][0]) - exact) <= slack and by[r][0] >= by[eu][0] - slack, r
                if rate > 0.0:
                    assert abs(by[r][0] - by[eu][0]) <= slack, r
            else:
                assert by[r][0] >= by[eu][0] - slack, r
                assert by[r][0] >= max(K - S0, 0.0) - slack, r
