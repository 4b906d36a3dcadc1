"""The lognormal reference (oracle/lognormal_exact.py: the exact terminal law with its dual rules, and the GBM-process
grid, in mpmath at 50 digits) on the committed cases (tests/golden/lognormal_exact.json), and the C oracle
(oracle/hh_oracle.c) held to it PER PATH at the bars of tests/euler_tangent_cases.py: hho_mc_solve on the exact law
(P = 8, REPLAY normals) — S_T, the price contribution and all eight partials of every usable path of every case — and
hho_gbm_grid, every row of every path.  The reference's partials are checked against the closed forms derived by hand in
its docstring.  The module prints the paths it left out per case and its worst error/bar per kind of comparison (`-s`).

Worst error/bar when this was written: 0.050 per path (S_T, bench), 0.027 on a sum, 0.016 on a grid row; no path left out."""
import os

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from oracle import lognormal_exact as lx  # noqa: E402
from oracle import lsm_oracle  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import lognormal_exact_cases as lc  # noqa: E402
from tests.lognormal_exact_cases import BY_ID, IDS, NS, SLOTS  # noqa: E402

GRID_STEPS = (1, 2, 7, 30)


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("lognormal_exact (C oracle)")
    yield w
    w.report()


def _oracle_solve(oracle, case, strike, cp, paths):
    res, term, _ = oracle.mc_solve(lc.model_of(case, strike, cp), lc.config_of(case, paths), n_threads=1)
    return res, term


def test_the_file_is_small_and_complete():
    assert os.path.getsize(lc.GOLDEN) < 100_000
    assert {c["tag"] for c in lc.CASES} == {"ref", "bench", "tiny-sigma", "sigma0", "short", "scale-small", "scale-large"}
    for tag in {c["tag"] for c in lc.CASES}:
        assert {(c["compat_sqrt_alpha"], c["antithetic"]) for c in lc.CASES if c["tag"] == tag} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for c in lc.CASES:
        strikes = {K for K, _ in c["payoff_list"]}
        assert sorted(c["payoff_list"]) == sorted((K, cp) for K in strikes for cp in (1.0, -1.0))
        assert strikes == ({50.0, 100.0, 300.0} if c["tag"] == "bench" else {c["S0"] if c["tag"] != "sigma0" else 100.0})
        z = np.array(c["z"])
        assert len(z) == 32 and np.array_equal(z * 2.0**40, np.rint(z * 2.0**40))  # multiples of 2^-40: exact doubles
        assert 8.5 in z and -8.5 in z and np.sum((z != 0) & (np.abs(z) < 2.0**-30)) == 2
        zeros = z[z == 0]
        assert sorted(np.signbit(zeros)) == [False, True]  # 0.0 and -0.0
    ref, bench = BY_ID["ref"], BY_ID["bench"]
    assert (ref["S0"], ref["sigma"], ref["r_drift"], ref["T"]) == (1.0, 1.0, 0.03, 366 / 365)
    assert (bench["S0"], bench["sigma"], bench["r_drift"], bench["T"]) == (100.0, 0.2, 0.05, 1.0)
    assert BY_ID["tiny-sigma"]["sigma"] == 1e-8 and BY_ID["sigma0"]["sigma"] == 0.0
    assert BY_ID["short"]["T"] == 1 / 365 and BY_ID["short"]["r_drift"] == -0.01
    assert {BY_ID["scale-small"]["S0"], BY_ID["scale-large"]["S0"]} == {1e-3, 1e6}


@pytest.mark.parametrize("name", IDS)
def test_digest_and_left_out_paths(name):
    """The reference module still computes what it computed when the cases were written (30 digits of the 50-digit sum
    per payoff and slot); the paths left out as undecided are within the project's cap — for these inputs the
    reference alone leaves out none."""
    case = BY_ID[name]
    ref = lc.reference(case)
    for j, pj in enumerate(ref["payoffs"]):
        left_out = int((~pj["usable"]).sum())
        print(f"\n{name} K={pj['strike']:g} cp={pj['cp']:+.0f}: {left_out} of {ref['n']} paths left out")
        assert left_out <= etc.MAX_UNUSABLE * ref["n"], (name, j)
        paths = lc.usable_paths(ref, j)
        with mp.workdps(lx.DPS):
            got = [mp.nstr(mp.fsum(pj["price"][i][s] for i in paths), 30) for s in range(1 + NS)]
        assert got == case["digests"][j], (name, j)


@pytest.mark.parametrize("name", IDS)
def test_reference_partials_are_the_closed_forms(name):
    """The dual rules against the hand derivation of oracle/lognormal_exact.py's docstring, at 50 digits: 1e-45 relative
    to the largest term of each form; the V0, κ, θ columns and everything out of the money are exact zeros."""
    case = BY_ID[name]
    ref = lc.reference(case)
    with mp.workdps(lx.DPS):
        S0, sig, r, T, D = (mp.mpf(case[k]) for k in ("S0", "sigma", "r_drift", "T", "discount"))
        s = mp.sqrt(T)
        m = s if case["compat_sqrt_alpha"] else T
        for j, (K, cp) in enumerate(case["payoff_list"]):
            pj = ref["payoffs"][j]
            for i, zf in enumerate(case["z"]):
                want = [mp.mpf(0)] * (1 + NS)
                for member in range(ref["members"]):
                    sz = s * mp.mpf(zf) * (-1 if member else 1)
                    S = mp.exp(mp.log(S0) + (r - sig * sig / 2) * m + sig * sz)
                    assert abs(S - ref["S"][member][i]) <= mp.mpf(10) ** -45 * S
                    if cp * (S - K) > 0:
                        dx = {"S0": 1 / S0, "sigma": -sig * m + sz, "r_drift": m}
                        row = [D * cp * (S - K)] + [D * cp * S * dx.get(slot, 0) for slot in SLOTS]
                        row[1 + SLOTS.index("discount")] = cp * (S - K)
                        row[1 + SLOTS.index("strike")] = -D * cp
                        want = [a + b / ref["members"] for a, b in zip(want, row)]
                for slot, got, w in zip(("price",) + SLOTS, pj["price"][i], want):
                    assert abs(got - w) <= mp.mpf(10) ** -45 * (abs(w) + D * (S + K) * (1 + abs(sig * m) + abs(s * zf))), (i, slot)
                    if slot in lc.ZERO_SLOTS or not any(want):
                        assert got == 0, (i, slot)


@pytest.mark.parametrize("name", IDS)
def test_bars_are_fp64_sized(name):
    """tests/test_euler_tangent_exact_host.py::test_bars_are_fp64_sized on this law, at its limit for short paths
    (1e-9): medians at most 1e-11·|value|, every bar below 1e-9·max(|value|, the slot's median), S_T bars below
    1e-10·S_T.  (The grid's bars: test_c_oracle_grid.)
    One slot is held against another scale: the antithetic σ-partial at σ = 1e-8 is D·(S⁺·(−σm + √T·z) + S⁻·(−σm − √T·z))/2
    with S⁺ = S⁻ to 1e-8 — the difference the case is there for.  It cancels to 1e-8 of its terms on EVERY path, so no
    path's value and no median shows the size of what was subtracted; the plain run's σ-partial of the same path is
    that size, and the bar is held to 1e-9 of it."""
    case = BY_ID[name]
    ref = lc.reference(case)
    cancelled = case["tag"] == "tiny-sigma" and case["antithetic"]
    etc.assert_bars_are_fp64_sized(ref, int(case["antithetic"]), 1e-9, skip=("sigma",) if cancelled else ())
    if cancelled:
        plain = lc.reference(BY_ID[name[:-len("-anti")]])
        s = 1 + SLOTS.index("sigma")
        for pj, pp in zip(ref["payoffs"], plain["payoffs"]):
            terms = np.array([abs(float(row[s])) for row in pp["price"]])
            if terms.any():
                bars = etc.path_bar(pj["price_e64"], pj["price_A"])[:, s]
                assert np.all(bars <= 1e-9 * np.maximum(terms, np.median(terms[terms > 0])))


def _grid_normals(oracle, n_steps):
    return np.array([[oracle.normal_pair(int(seed), s >> 1)[s & 1] for s in range(n_steps)] for seed in lc.GRID_SEEDS])


@pytest.mark.parametrize("n_steps", GRID_STEPS)
@pytest.mark.parametrize("name", IDS)
def test_c_oracle_grid(oracle, worst, name, n_steps):
    """hho_gbm_grid on 32 keys against the grid reference evaluated on the normals it draws (oracle.normal_pair: the
    same function, the same doubles), every row of every path; the flipped-σ ensemble when the case is antithetic.  The
    grid reads neither compat_sqrt_alpha nor the payoffs: the four cases of a model share two references."""
    case = BY_ID[name]
    z = _grid_normals(oracle, n_steps)
    ref = lc.grid_reference(case, n_steps, case["T"], z)
    W = np.array([[[float(w) for w in rows] for rows in mem] for mem in ref["W"]])
    # fp64-sized: A gains about 2·|W| per date, so after k dates it is some (2k + 1) times the LARGEST W the path has had
    assert np.all(etc.path_bar(ref["e64"], ref["A"]) <= 1e-11 * np.maximum.accumulate(W, axis=2))
    got = lsm_oracle.gbm_grid(lc.GRID_SEEDS, n_steps, case["S0"], case["r_drift"], case["sigma"], case["T"], case["antithetic"])
    bad = lc.check_grid(worst, "oracle", got, ref, case["antithetic"], f"{name} steps={n_steps}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", IDS)
def test_c_oracle_path_by_path(oracle, worst, name):
    """hho_mc_solve on the exact law as REPLAY with n_paths = 1, eight unit seeds: dprice[k] is the path's partial."""
    case = BY_ID[name]
    ref = lc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        for i in lc.usable_paths(ref, j):
            res, term = _oracle_solve(oracle, case, strike, cp, [i])
            bad += etc.check_solve(worst, case, ref, j, [i], res, term, "oracle")
            for slot in lc.ZERO_SLOTS:
                assert res.dprice[SLOTS.index(slot)] == 0.0, (name, i, slot)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", IDS)
def test_c_oracle_all_paths_in_one_call(oracle, worst, name):
    case = BY_ID[name]
    ref = lc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        paths = lc.usable_paths(ref, j)
        res, term = _oracle_solve(oracle, case, strike, cp, paths)
        assert res.n_paths_done == len(paths)
        bad += etc.check_solve(worst, case, ref, j, paths, res, term, "oracle")
    assert not bad, "\n".join(bad[:20])
