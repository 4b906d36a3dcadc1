"""The path-statistics family, bit for bit (tests/path_family_cases.py): every case's statistics, var_T and solve
results hash to what tests/golden/path_family_pins.json recorded.  The fixture holds for the toolchain it was recorded
with — another compiler may schedule the same source to other bits — and the module skips under any other one."""
import pytest

from tests import path_family_cases as pf

pytestmark = pytest.mark.gpu

DOC = pf.load_golden()


@pytest.fixture(scope="module")
def got(hhlib):
    assert DOC is not None, "tests/golden/path_family_pins.json is missing"
    here = pf.toolchain()
    if here != DOC["toolchain"]:
        pytest.skip(f"the pins were recorded with another toolchain: {DOC['toolchain']!r}, here {here!r}")
    return pf.compute(hhlib)


def test_the_fixture_covers_every_case_and_its_cases_take_every_branch():
    ids = [cid for cases in (pf.stat_cases(), pf.solve_cases()) for cid, _ in cases]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(DOC["pins"])
    assert DOC["n_paths"] == pf.N
    pf.check_seen(DOC["seen"])


@pytest.mark.parametrize("family", ["em", "merton", "qe", "bates", "assets", "solve"])
def test_bits_are_the_recorded_ones(got, family):
    mine = {k: v for k, v in got.items() if k.startswith(family + "/")}
    assert mine
    moved = [k for k, v in mine.items() if v != DOC["pins"][k]]
    assert not moved, f"{len(moved)} of {len(mine)} cases moved, the first: {moved[:8]}"
