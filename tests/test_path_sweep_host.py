"""The sweep over model values (tests/path_sweep_cases.py) on the host: the admissibility restatement against the header's
constants and the library's own texts; every digest of tests/golden/path_sweep.json reproduced by the restatements as
they stand; the unusable cap and the counts that show each case exercises its edge; how large the sweep's bars are
against the values they guard; and SENSITIVITY — every mutation of qe_cases and bates_cases, and the three that only a
sweep can see, puts the fp64 restatement outside a bar of some usable trajectory of some sweep case: the evidence that a
kernel wrong in that way would fail tests/test_gpu_path_sweep.py.  No GPU."""
import os
import re

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import bates_cases as bt  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import path_sweep_cases as sw  # noqa: E402
from tests import qe_cases as qc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = sw.DOC
RECORDS = {r["id"]: r for r in DOC["cases"]} if DOC else {}
ALL = [c for f in sw.FAMILIES for c in sw.cases(f)]

ILL_CONDITIONED = sw.ILL_CONDITIONED
E64_LIMIT = sw.FP64_SIZED   # euler_tangent_cases' figure: bars "below 1e-9 except where a partial has cancelled"


# ---- admissibility -------------------------------------------------------------------------------------------------------

def test_the_fixture_is_there_and_is_the_makers():
    assert DOC is not None and DOC["seed"] == sw.SEED and DOC["n_paths"] == sw.N_PATHS == 65 and DOC["cap"] == sw.CAP == 1
    assert set(DOC["drawn"]) == set(sw.FAMILIES) and all(len(v) == sw.DRAWN_BY_FAMILY.get(f, sw.DRAWN_N) for f, v in DOC["drawn"].items())
    assert sorted(RECORDS) == sorted(sw.case_id(c) for c in ALL) and len(RECORDS) == len(ALL)
    assert os.path.getsize(sw.GOLDEN) < 2 ** 20


def test_the_restatement_uses_the_headers_constants_and_the_librarys_texts():
    hdr = open(os.path.join(ROOT, "include", "hedgehog_mc.h")).read()
    assert re.search(r"#define HH_QE_MAX_PSI\s+1e9\b", hdr) and sw.MAX_PSI == 1e9
    assert re.search(r"#define HH_JUMP_MAX_MEAN\s+64\.0\b", hdr) and sw.MAX_MEAN == 64.0
    api = open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_api.hip")).read()
    texts = {t for f in sw.FAMILIES for _, _, _, _, t in sw.rejected(f)}
    assert len(texts) >= 9
    for t in texts:
        assert t in api, t


@pytest.mark.parametrize("family", sw.FAMILIES)
def test_every_edge_row_is_admitted_and_its_neighbour_outside_is_not(family):
    """on every step count a row runs at; the drawn models at theirs"""
    for case in sw.EDGE[family]:
        for n_steps, _ in (sw.SHAPES if family != "merton_terminal" else ((1, 1),)):
            assert sw.defect(case, n_steps) is None, (sw.case_id(case), n_steps)
    for case in sw.cases(family)[len(sw.EDGE[family]):]:
        assert sw.defect(case, sw.DRAWN_SHAPE[0]) is None, sw.case_id(case)
    names = [name for name, *_ in sw.rejected(family)]
    assert len(set(names)) == len(names) >= 3
    for name, case, n_steps, code, text in sw.rejected(family):
        assert sw.defect(case, n_steps) == (code, text), name


def test_the_edge_table_has_the_rows_the_issue_lists():
    qe = {c["name"]: c for c in sw.EDGE["qe"]}
    assert {qe[n]["model"]["rho"] for n in ("rho_+0.6", "rho_0", "rho_-1", "rho_+1")} == {0.6, 0.0, -1.0, 1.0}
    assert all(qe[n]["mart"] == 0 for n in qe if qe[n]["model"]["rho"] > 0)
    assert {c["psi_c"] for c in qe.values()} >= {1.0, 2.0, 1.25} and qe["V0_0"]["model"]["V0"] == 0.0
    ratio = lambda m: m["sigma"] ** 2 / (2 * m["kappa"] * m["theta"])  # noqa: E731
    assert 0.999e6 < ratio(qe["psi_max_1e6"]["model"]) <= 1e6 and 0.9899e9 < ratio(qe["psi_max_0.99e9"]["model"]) <= 0.99e9
    bates = sw.EDGE["bates"]
    assert {c["mean"] for c in bates} >= {0.0, 1e-3, 8.0, 64.0} and {c["mu_j"] for c in bates} >= {-2.0, 1.0}
    assert any(c["sigma_j"] == 0.0 for c in bates) and {c["model"]["rho"] for c in bates} >= {0.6, 0.0, -1.0, 1.0}
    assert {c["psi_c"] for c in bates} >= {1.0, 2.0, 1.25}
    for fam in ("merton_path", "merton_terminal"):
        rows = sw.EDGE[fam]
        assert {c["mean"] for c in rows} >= {0.0, 1e-3, 2.5, 8.0, 64.0} and {c["mu_j"] for c in rows} >= {-2.0, 1.0}
        assert any(c["sigma_j"] == 0.0 for c in rows) and {c["model"]["sigma"] for c in rows} >= {1e-8, 2.0}
    assets = sw.EDGE["assets"]
    assert {len(c["model"]["spots"]) for c in assets} == {1, 2, 3, 8} and {c["kind"] for c in assets} == set(sw.ac.KINDS)
    assert {c["model"]["corr"][0][1] for c in assets if len(c["model"]["spots"]) == 2} >= {0.999, -0.999}
    sums = [c for c in assets if c["kind"] == sw.ac.SUM]
    assert any(0.0 in c["model"]["weights"] for c in sums) and any(min(c["model"]["weights"]) < 0.0 for c in sums)
    assert any(0.0 in c["model"]["sigmas"] for c in assets)
    eu = {c["name"]: c for c in sw.EDGE["euler"]}
    assert {c["model"]["sigma"] for c in eu.values() if c["dynamics"] == "lognormal"} == {1e-8, 2.0}
    for tag, split in (("split", 1), ("classic", 0)):
        assert all(eu[f"{tag}_{k}"]["em_split"] == split for k in ("rho_+1", "rho_-1", "rho_0", "vol_of_vol_below_0", "V0_0", "clipped"))
        assert eu[f"{tag}_vol_of_vol_below_0"]["model"]["sigma"] < 0 and eu[f"{tag}_V0_0"]["model"]["V0"] == 0.0
    lv = sw.EDGE["localvol"]
    for name in sw.lc.SURFACES:
        assert {f"{name}_S0_{k}" for k in ("lowest_node", "highest_node", "off_grid")} <= {c["name"] for c in lv}
    assert any(c["model"]["r_drift"] < 0 for c in lv)
    assert any(c["model"]["T"] < sw.lc.surface(c["surface"])["times"][0] for c in lv)
    assert any(c["model"]["T"] > sw.lc.surface(c["surface"])["times"][-1] and len(sw.lc.surface(c["surface"])["times"]) > 1 for c in lv)
    assert sw.TERMINAL_OFFSETS == (0, 2 ** 33 - 1) and sw.TERMINAL_SIZES == (1, 63, 65)


def test_the_drawn_models_are_the_streams(oracle):
    """the stored hex floats are the first draws of draw_models that stay within the cap (none was passed over, so they
    are its first DRAWN_N), up to the last bit of this machine's exp"""
    for family in sw.FAMILIES:
        stream = sw.draw_models(family)
        for rec in DOC["drawn"][family]:
            stored, drawn = sw.from_hex(rec), next(stream)
            assert stored["name"] == drawn["name"] and stored.get("mart") == drawn.get("mart")
            assert stored.get("kind") == drawn.get("kind")
            for k, v in stored["model"].items():
                np.testing.assert_allclose(np.array(v), np.array(drawn["model"][k]), rtol=1e-13, atol=0, err_msg=f"{family} {stored['name']} {k}")


# ---- digests, the cap, the counts, the bars ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bar_report():
    """the table a reader needs, printed at the module's end (`-s`): per family the largest bar against its path's scale
    and how many cases lie above 1e-9; the ill-conditioned rows with their reason"""
    seen = {}
    yield seen
    for family in sw.FAMILIES:
        mine = {k: v for k, v in seen.items() if k.startswith(family + ":")}
        if mine:
            top = max(mine, key=lambda k: mine[k][0])
            print(f"\nsweep bars, {family}: largest path_bar/scale {mine[top][0]:.3g} ({top} {mine[top][1]}); "
                  f"{sum(v[0] > 1e-9 for v in mine.values())} of {len(mine)} cases above 1e-9 and narrowed to it")
    for k, why in ILL_CONDITIONED.items():
        if k in seen:
            print(f"\nill-conditioned by construction: {k}: bar/scale {seen[k][0]:.3g} — {why}")


@pytest.mark.parametrize("case", ALL, ids=sw.case_id)
def test_digests_counts_cap_and_bars(oracle, bar_report, case):
    rec = RECORDS[sw.case_id(case)]
    walks = {key: sw.walk(oracle, case, key) for key, _ in sw.shapes_of(case)}
    sw.check_expectations(case, walks)   # the cap and what the case is for
    worst = (0.0, None)
    for key, every, start in sw.combos(case):
        ref = sw.reference(case, walks[key], every, start)
        assert sw.digest(ref, walks[key]["usable"]) == rec["digests"][f"{key}x{every}+{start}"], (key, every, start)
        u = walks[key]["usable"]
        scale = sw.scales(ref)[:, u]
        assert np.all(np.isfinite(ref["e64"])) and np.all(np.isfinite(ref["A"]))
        wide, held = etc.path_bar(ref["e64"], ref["A"])[:, u], sw.bars(case, ref)[:, u]
        ratio = float(np.max(wide / np.where(scale > 0, scale, 1.0)))
        if ratio > worst[0]:
            worst = (ratio, f"{key}x{every}+{start}")
        if sw.case_id(case) not in ILL_CONDITIONED:
            # the fp64 restatement keeps a factor 20 inside the bar the device is held to, and that bar is fp64-sized
            assert np.all(etc.FACTOR * ref["e64"][:, u] <= E64_LIMIT * scale), (key, every, start)
            assert np.all(held <= E64_LIMIT * scale) and np.all(held <= wide), (key, every, start)
        else:
            # held to the fp64 restatement instead (tests/test_gpu_path_sweep.py): it is there, finite, and the reason
            # for the exemption is e64 itself, not the magnitude rule
            assert np.all(np.isfinite(ref["f64"])) and np.any(etc.FACTOR * ref["e64"][:, u] > E64_LIMIT * scale) or key == 1
    bar_report[sw.case_id(case)] = worst
    sw.check_expectations(case, walks)   # again: local volatility counts its off-grid states in the reference
    for key, w in walks.items():
        assert sw.json_counts(w["counts"]) == rec["counts"][str(key)], key


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------

def _case(family, name):
    return next(c for c in sw.EDGE[family] if c["name"] == name)


def _misses(oracle, case, mut, key=5, every=1, start=1):
    """how many (member, usable trajectory, row) of the fp64 restatement mutated by `mut` lie outside the case's bars"""
    w = sw.walk(oracle, case, key)
    ref = sw.reference(case, w, every, start)
    bars = sw.bars(case, ref)
    if case["family"] == "bates" and mut in ("odd_words", "mean_T"):
        d, jm = sw.draws(oracle, "bates", key), sw.jump_model(case, key)
        N = np.array([bt.mutated_counts(jm, key, d["UJ"][i], mut) for i in range(sw.N_PATHS)])
        runs, _ = bt.walks(jm, key, d, N, 1, case["mart"], check=False, psi_c=case["psi_c"])
    else:
        runs = sw.walk(oracle, case, key, mut=mut)["runs"]
    out = 0
    with mp.workdps(qc.DPS):
        for m in range(2):
            for i in np.flatnonzero(w["usable"]):
                _, _, xs, vT = runs[m][i]
                got = qc.rows_of(case["model"], xs, float, every, start) + [vT]
                out += sum(abs(mp.mpf(got[row].v) - ref["want"][m][i][row]) > bars[m][i][row] for row in range(6))
    return out


QE_SENSITIVE = ("psi_c_1.25", "psi_c_2.0", "rho_-1")
BATES_SENSITIVE = ("psi_c_2.0_mean_0.9", "rho_+0.6_mean_8")


def test_unmutated_the_restatement_is_inside_every_bar(oracle):
    for fam, names in (("qe", QE_SENSITIVE), ("bates", BATES_SENSITIVE)):
        for name in names:
            assert _misses(oracle, _case(fam, name), None) == 0, (fam, name)


@pytest.mark.parametrize("mut", qc.MUTATIONS)
def test_a_sweep_case_catches_every_qe_mutation(oracle, mut):
    found = {name: _misses(oracle, _case("qe", name), mut) for name in QE_SENSITIVE}
    print(f"\n{mut}: (member, trajectory, row) outside the bars: {found}")
    assert max(found.values()) > 0, found


@pytest.mark.parametrize("mut", bt.MUTATIONS)
def test_a_sweep_case_catches_every_bates_mutation(oracle, mut):
    found = {name: _misses(oracle, _case("bates", name), mut) for name in BATES_SENSITIVE}
    print(f"\n{mut}: (member, trajectory, row) outside the bars: {found}")
    assert max(found.values()) > 0, found


def test_the_sweeps_own_mutations_are_caught_where_the_issue_says(oracle):
    """ψ_c ignored: by a ψ_c ∈ {1, 2} case — and by no case at the default; the root's argument floored: by a ρ = ±1 case
    (with |ρ| < 1 only a state that stays at v = v′ = 0 meets the floor); N for √N: by a case with N >= 2"""
    assert qc.SWEEP_MUTATIONS == ("psi_fixed", "var_floor", "sqrt_N")
    for name in ("psi_c_1.0", "psi_c_2.0"):
        assert _misses(oracle, _case("qe", name), "psi_fixed") > 0, name
    assert _misses(oracle, _case("qe", "rho_+0.6"), "psi_fixed") == 0
    for name in ("rho_-1", "rho_+1", "rho_-1_plain"):
        assert _misses(oracle, _case("qe", name), "var_floor") > 0, name
    for name in ("rho_+0.6_mean_8", "rho_-1_mean_64"):
        case = _case("bates", name)
        assert max(sw.walk(oracle, case, 5)["counts"]["N"]) >= 2
        assert _misses(oracle, case, "sqrt_N") > 0, name
    assert _misses(oracle, _case("bates", "rho_+1_mean_8_sigma_j_0"), "sqrt_N") == 0   # σ_J = 0: √N multiplies 0
    assert _ffi.HH_JUMP_MAX_COUNT == 255
