"""hedgehog.jl_amd/csrc/hh_layout.h (where the LSM, Broadie–Kaya and grid-sort scratch buffers are carved) compiled
for the HOST with g++ and compared, offset by offset, with tests/golden/scratch_layouts.json.

The golden numbers are those of the commit BEFORE the layouts had one definition (525513d): a one-off program held
that commit's lsm_layout / lsm_scratch_doubles, bk_*_offset / bk_scratch_bytes / bk_prepare / bk_diag_ptrs /
bk_live_records and bk_grid_sort_bytes / launch_bk_grid carving verbatim (sizeof(BkArgs) and sizeof(BkTables) made
inputs), applied them to a fake base address and printed the pointer differences; hh_api.hip's "from the end"
expressions gave `counters` and `stamps`.  Nothing in the file was computed by hh_layout.h: a region that moves
shows here before it shows as an out-of-bounds write on a device."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import host_cxxflags, host_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every rounding edge: tile counts on both sides of kHeavyGrid = 64 and kSlots = 1536 tiles, multiples of 4 and
# not; chunk rules on both sides of 2^18, 2^19, 2^20; the sort's runs of 1024
BK_SHAPES = list(itertools.product([1, 256, 257, 600, 16384, 16385, 393216, 393217, 1 << 22], [0, 8, 1024],
                                   [(1, 1), (4096, 100000), (1, 100000), (4096, 1)]))
LSM_SHAPES = list(itertools.product([1, 1024, 1025, 1 << 18, (1 << 18) + 1, (1 << 19) + 1, (1 << 20) + 1, 1 << 21],
                                    [1, 2, 100, 1023, 1024], [1, 3, 8]))
SORT_SHAPES = [1 << 20, (1 << 20) + 1, 2_400_000, 1 << 22]
N_KEY = {"lsm": 3, "bk": 4, "sort": 1}  # leading fields that name the shape
# regions in the order they lie in memory; `total` closes the last one
ORDER = {"lsm": ["sync", "ring", "rec_stats", "rowstat", "rec_pow", "P", "recB", "disc_pow", "counters", "stamps", "total"],
         "bk": ["long_mask", "slot_lines", "counters", "args", "tables", "phi_cache", "draws", "iv", "diag", "total"],
         "sort": ["perm", "counts", "totals", "keys", "total"]}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "scratch_layouts.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """{kind: {shape: {field: value}}} as hh_layout.h computes them for every shape of the lists above"""
    exe = tmp_path_factory.mktemp("layout") / "layout_check"
    subprocess.run(["g++", *host_cxxflags(), "-std=c++17", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "hedgehog.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "layout_check.cpp"), "-o", str(exe)], check=True)
    req = [f"lsm {n} {s} {d}" for n, s, d in LSM_SHAPES]
    req += [f"bk {n} {c} {sa} {st}" for n, c, (sa, st) in BK_SHAPES]
    req += [f"sort {n}" for n in SORT_SHAPES]
    out = subprocess.run([str(exe)], input="\n".join(req) + "\n", check=True, capture_output=True, text=True,
                         env=host_env()).stdout
    lines = out.strip().splitlines()
    assert len(lines) == len(req)
    return [(ln.split()[0], [int(w) for w in ln.replace(":", " ").split()[1:]]) for ln in lines]


pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def as_dicts(golden, layouts):
    out = {k: {} for k in N_KEY}
    for kind, row in layouts:
        fields = golden[kind]["fields"]
        assert len(row) == len(fields)
        out[kind][tuple(row[:N_KEY[kind]])] = dict(zip(fields, row))
    return out


def test_layouts_are_where_they_were(golden, layouts):
    got = as_dicts(golden, layouts)
    for kind, g in golden.items():
        want = {tuple(r[:N_KEY[kind]]): dict(zip(g["fields"], r)) for r in g["rows"]}
        assert set(want) == set(got[kind]), kind  # the golden file covers exactly the shapes listed above
        for shape, w in want.items():
            assert got[kind][shape] == w, (kind, shape)
    assert len(got["lsm"]) == len(LSM_SHAPES) and len(got["bk"]) == len(BK_SHAPES) and len(got["sort"]) == len(SORT_SHAPES)


def test_hand_derived_offsets(golden, layouts):
    """three shapes worked out by hand from the expressions the layouts replaced"""
    got = as_dicts(golden, layouts)
    lsm = got["lsm"][(1024, 1, 1)]
    assert (lsm["total"], lsm["counters"], lsm["rec_stats"]) == (262186, 262176, 262146)
    bk = got["bk"][(600, 0, 1, 1)]
    assert (bk["slot_lines"], bk["counters"] + 4, bk["args"], bk["cache_columns"]) == (128, 1156, 1280, 16384)
    assert bk["total"] - bk["draws"] == 36864  # 768 lanes x 48 bytes
    assert got["sort"][(1 << 20,)]["total"] == 6292736


def test_regions_are_ordered_disjoint_and_aligned(golden, layouts):
    for kind, by_shape in as_dicts(golden, layouts).items():
        for shape, s in by_shape.items():
            at = [s[name] for name in ORDER[kind]]
            assert at[0] == 0 and all(a < b for a, b in zip(at, at[1:])), (kind, shape, at)  # no region is empty
            if kind == "lsm":
                ntot, n_steps, degree = shape
                rows, ch, nv = n_steps + 1, s["nch"], 2 * degree + 1
                assert s["nch"] == -(-ntot // (512 * s["q"])) and s["rows"] == rows
                size = [2, 16 * 256 * 32 * 2, rows * ch * 3, rows * 3, rows * ch * nv, rows * nv,
                        rows * ch * (degree + 1), rows, 2, 8]
                # contiguous: each region ends where the next starts, `total` is the end of the last
                assert [b - a for a, b in zip(at, at[1:])] == size, (shape, at)
            elif kind == "bk":
                n_chain, term_cache, sizeof_args, sizeof_tables = shape
                lanes = s["lanes"]
                assert lanes == -(-n_chain // 256) * 256 and s["cache_cap"] == (term_cache or 256)
                assert s["slot_lines"] % 128 == 0 and s["args"] % 256 == 0 and s["tables"] % 256 == 0
                size = [lanes // 64 * 8, 8 * 128, 128, sizeof_args, sizeof_tables, s["cache_columns"] * s["cache_cap"] * 8,
                        4 * lanes * 8, lanes * 8, 2 * lanes * 4]
                gaps = [b - a - n for a, b, n in zip(at, at[1:], size)]
                assert all(0 <= g < 256 for g in gaps) and gaps[5:] == [0, 0, 0, 0], (shape, at, gaps)
            else:
                lanes = -(-shape[0] // 256) * 256
                assert s["n_runs"] == -(-shape[0] // 1024)
                assert [b - a for a, b in zip(at, at[1:])] == [lanes * 4, 256 * s["n_runs"] * 4, 1024, lanes + 256]
