"""Every Monte Carlo route of the Python host against tests/golden/route_pins.json, without a GPU: the entry points
reached, every struct and scalar passed, the order of the solutions, and every refusal's type and text, recorded before
the routes were stated in one table (tests/route_cases.py has the recorder and the cases; the file holds a SHA-256 per
record and the refusal texts)."""
import pytest

from tests import route_cases as rc

DOC = rc.load_golden()


@pytest.fixture(scope="module")
def records():
    return rc.compute()


def test_every_record_is_the_pinned_one(records):
    now = rc.pins(records)
    assert {g: sorted(d) for g, d in now["pins"].items()} == {g: sorted(d) for g, d in DOC["pins"].items()}  # exactly the cases
    differing = [f"{g}/{t}" for g, d in DOC["pins"].items() for t in d if now["pins"][g][t] != d[t]]
    for cid in differing[:5]:
        print(cid, "\n  now:", records[cid])
    assert differing == [] and now["messages"] == DOC["messages"]


def test_a_refusal_touches_no_device(records):
    refusals = [cid for cid, r in records.items() if "raises" in r]
    assert len(refusals) > 300 and all(records[cid]["calls"] == [] for cid in refusals)


def test_the_table_covers_what_it_says(records):
    """every route with ensemble and antithetic on and off, every entry point of the family, the 7-row statistics, a
    MethodError and a ValueError from every path route, None from solve_montecarlo_many wherever there is no
    hh_mc_solve_multi form"""
    entries = {c["entry"] for r in records.values() for c in r["calls"]}
    assert entries >= {"hh_mc_solve", "hh_mc_solve_multi", "hh_mc_solve_basket", "hh_mc_solve_jump", "hh_mc_solve_path",
                       "hh_mc_solve_path_ex", "hh_mc_solve_path_jump", "hh_mc_solve_path_qe", "hh_mc_solve_path_bates",
                       "hh_mc_solve_path_lv", "hh_mc_solve_path_assets"}
    for name, r in rc.ROUTES.items():
        for ens in (False, True):
            for anti in (False, True):
                rec = records[f"{name}/single/good/ensemble={ens}/antithetic={anti}"]
                assert len(rec["calls"]) == 1 and (rec["out"]["ensemble"] is not None) == ens, (name, ens, anti)
        kinds = {rec["raises"][0] for cid, rec in records.items() if cid.startswith(name + "/fault/") and "raises" in rec}
        assert "MethodError" in kinds and (not r["path"] or "ValueError" in kinds), name
        assert (records[f"{name}/many/good"]["out"] is None) == (name not in ("plain", "plain_euler")), name
    bridge = records["euler/single/continuous_barrier/ensemble=True/antithetic=True"]
    assert bridge["out"]["ensemble"] == {"shape": [7, 16], "given": True} and bridge["calls"][0]["entry"] == "hh_mc_solve_path_ex"
