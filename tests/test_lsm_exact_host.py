"""oracle/lsm_exact.py on the CPU: the exact reference recovers what a least-squares fit must give (exact
polynomial data, per-value means, interpolation), and an fp64 restatement of the device's row fit — rowstat_of,
the power and moment sums in the device's summation tree, solve_normal_equations_wave with its drop rule, Horner
in z — stays within the derived margin δ on random and hand-made rows.  The bound is shown here, not tuned to a
GPU run: test_gpu_lsm_exact.py uses it unchanged."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import lsm_exact as L


def test_exact_sum_is_exact():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(20_000) * np.exp(rng.uniform(-40, 40, 20_000))
    a = np.concatenate([a, -a[:5000], [0.0, 1e300, -1e300, 5e-324]])
    want = sum((Fraction(float(v)) for v in a), Fraction(0))
    assert L.exact_sum(a) == want
    assert float(L.exact_sum(a)) == math.fsum(a)


def test_power_sums_are_exact():
    z = np.array([0.1, -3.0, 2.5, 1e-3, 7.0 / 3.0])
    y = np.array([1.5, -0.25, 3.0, 2.0, 1.0 / 3.0])
    with L.mpmath.workdps(400):
        P = L.exact_power_sums(z, kmax=16)
        B = L.exact_power_sums(z, y, kmax=8)
        for m in range(17):
            want = sum(Fraction(v) ** m for v in z)
            assert abs(P[m] - L.mpmath.mpf(want.numerator) / want.denominator) <= L.mpmath.mpf(10) ** -300 * abs(P[m])
        for k in range(9):
            want = sum(Fraction(v) ** k * Fraction(w) for v, w in zip(z, y))
            assert abs(B[k] - L.mpmath.mpf(want.numerator) / want.denominator) <= L.mpmath.mpf(10) ** -300 * abs(B[k])


def test_tree_sum_matches_its_depth():
    rng = np.random.default_rng(5)
    for ntot in (1, 511, 1025, 2 ** 18 + 1):
        t = rng.standard_normal(ntot)
        got = L.tree_sum(t)
        h = L.tree_depth(ntot)
        assert abs(got - float(L.exact_sum(t))) <= h * L.U * np.sum(np.abs(t))


@pytest.mark.parametrize("degree", range(1, 9))
def test_reference_recovers_polynomial_data(degree):
    rng = np.random.default_rng(degree)
    x = 100.0 * np.exp(0.3 * rng.standard_normal(400))
    z = (x - 100.0) / 30.0
    c = rng.standard_normal(degree + 1)
    y = sum(ck * z ** k for k, ck in enumerate(c))
    fit = L.exact_row_fit(x, y, degree, h=1)
    # y holds rounding of its own (fp64 Horner), so the exact fit reproduces it to that rounding
    assert np.max(np.abs(fit.fitted - y)) <= 1e-12 * np.max(np.abs(y))


@pytest.mark.parametrize("degree", [1, 3, 5, 8])
@pytest.mark.parametrize("m", [1, 2, 3, 9])
def test_reference_on_repeated_spots_gives_per_value_means_or_interpolates(degree, m):
    rng = np.random.default_rng(10 * degree + m)
    levels = 100.0 + np.arange(m) * 1.25
    x = levels[rng.integers(0, m, 500)]
    y = rng.uniform(0, 10, 500)
    fit = L.exact_row_fit(x, y, degree, h=1)
    if m <= degree + 1:   # the fit passes through every per-value mean
        for v in levels:
            sel = x == v
            if sel.any():
                mean = float(L.exact_sum(y[sel]) / int(sel.sum()))
                assert np.allclose(fit.fitted[sel], mean, rtol=1e-13, atol=0)
        assert len(fit.kept) == min(m, degree + 1) and not fit.ambiguous
    # few paths on distinct spots: interpolation
    xs = 90.0 + rng.uniform(0, 5, min(m, degree + 1))
    ys = rng.uniform(0, 10, len(xs))
    fi = L.exact_row_fit(xs, ys, degree, h=1)
    np.testing.assert_allclose(fi.fitted, ys, rtol=1e-12)


def _random_row(rng, degree):
    sigma, T, n = rng.uniform(0.05, 0.8), rng.uniform(0.05, 3.0), int(rng.choice([2, 5, 30, 200, 1000]))
    S0, cp = rng.uniform(20, 200), rng.choice([1.0, -1.0])
    K = S0 * rng.uniform(0.6, 1.5)
    x = S0 * np.exp(sigma * math.sqrt(T) * rng.standard_normal(n))
    x = x[cp * (x - K) > 0]
    sN = x * np.exp(sigma * math.sqrt(T / 4) * rng.standard_normal(len(x)))
    y = 0.98 * np.maximum(cp * (sN - K), 0.0)
    return x, y, cp * (x - K)


def _check_rows(rows, report):
    worst, inside, total, decided_flips = 0.0, 0, 0, 0
    for x, y, pay, degree in rows:
        f, _, _ = L.device_row_fit(x, y, degree)
        fit = L.exact_row_fit(x, y, degree, h=L.tree_depth(len(x)))
        err = np.abs(f - fit.fitted)
        assert np.all(err <= fit.delta), (degree, len(x), float(np.max(err / fit.delta)))
        if len(x) and np.all(np.isfinite(fit.delta)):
            worst = max(worst, float(np.max(err / np.where(fit.delta > 0, fit.delta, 1.0))))
        ex, near = L.decisions(pay, fit)
        decided_flips += int(np.sum(((pay > f) != ex) & ~near))
        inside += int(near.sum())
        total += len(x)
    print(f"\n{report}: worst |fp64 fit − exact| / δ = {worst:.3g}; {inside} of {total} decisions inside δ")
    assert decided_flips == 0
    return worst, inside, total


def test_device_row_fit_stays_within_delta_on_random_rows():
    rng = np.random.default_rng(2024)
    rows = []
    while len(rows) < 240:
        degree = int(rng.integers(1, 9))
        x, y, pay = _random_row(rng, degree)
        rows.append((x, y, pay, degree))
    worst, inside, total = _check_rows(rows, "random rows")
    assert worst < 0.5 and inside <= 0.002 * total + 3


def test_device_row_fit_stays_within_delta_on_hand_made_rows():
    rng = np.random.default_rng(77)
    rows = []
    for degree in range(1, 9):
        for m in range(1, degree + 2):                      # 500 paths on 1 … D+1 distinct spots
            lv = 100.0 - 3.0 * np.arange(m)
            x = lv[rng.integers(0, m, 500)]
            y = rng.uniform(0, 20, 500)
            rows.append((x, y, 110.0 - x, degree))
        for n in range(0, degree + 2):                      # 0 … D+1 in-the-money paths
            x = 100.0 - rng.uniform(0, 20, n)
            rows.append((x, rng.uniform(0, 20, n), 110.0 - x, degree))
        x = np.full(300, 97.0)                              # all spots equal: var = 0
        rows.append((x, rng.uniform(0, 20, 300), 110.0 - x, degree))
        x = 100.0 * (1.0 + 1e-9 * rng.standard_normal(400))  # spread 1e-9 of the level
        rows.append((x, rng.uniform(0, 20, 400) + 50.0 * (x - 100.0) * 1e7, 110.0 - x, degree))
        x = 1e4 * np.exp(0.2 * rng.standard_normal(600))     # level 1e4
        x = x[x < 1.1e4]
        rows.append((x, np.maximum(1.1e4 - x * np.exp(0.1 * rng.standard_normal(len(x))), 0), 1.1e4 - x, degree))
        x = 4.6 + 0.05 * rng.standard_normal(800)            # log rows near 4.6
        x = x[x < 4.65]
        rows.append((x, np.maximum(4.65 - x - 0.02 * rng.standard_normal(len(x)), 0), 4.65 - x, degree))
    _check_rows(rows, "hand-made rows")
