"""The Carr–Madan entry points, bit for bit (tests/carr_madan_law_cases.py, part 2): every case's prices and gradients
hash to what tests/golden/carr_madan_pins.json recorded.  The fixture holds for the toolchain it was recorded with —
another compiler may schedule the same source to other bits — and the module skips under any other one."""
import pytest

from tests import carr_madan_law_cases as cl

pytestmark = pytest.mark.gpu

DOC = cl.load_golden()
ENTRIES = ["single", "basket", "grad", "jump", "bates", "vg"]


@pytest.fixture(scope="module")
def got(hhlib):
    assert DOC is not None, "tests/golden/carr_madan_pins.json is missing"
    here = cl.toolchain()
    if here != DOC["toolchain"]:
        pytest.skip(f"the pins were recorded with another toolchain: {DOC['toolchain']!r}, here {here!r}")
    return cl.compute(hhlib)


def test_the_fixture_covers_every_case():
    ids = [cid for cid, _ in cl.cases()]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(DOC["pins"])
    assert sorted({cid.split("/")[0] for cid in ids}) == sorted(ENTRIES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_bits_are_the_recorded_ones(got, entry):
    mine = {k: v for k, v in got.items() if k.startswith(entry + "/")}
    assert mine
    moved = [k for k, v in mine.items() if v != DOC["pins"][k]]
    assert not moved, f"{len(moved)} of {len(mine)} cases moved, the first: {moved[:8]}"
