"""Quasi-Monte Carlo on the host side, without a GPU: the three entry points declared, exported and bound; the direction
numbers against PyTorch's unscrambled engine for all 4096 dimensions; the committed table against its maker; the
Brownian-bridge table's properties; csrc/hh_sobol.h as a stand-alone host program (also under AddressSanitizer and UBSan)
against the Python restatement, bit for bit; the golden file's margins; how the Python layer routes and refuses."""
import ctypes as C
import importlib.util
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from hedgehog_jl_amd import qmc
from tests import sobol_cases as sc
from tests.conftest import host_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
CSRC = os.path.join(ROOT, "hedgehog.jl_amd", "csrc")
NEW = {"hh_sobol_directions": 2, "hh_sobol_points": 8, "hh_sobol_fill": 12}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------

def test_new_prototypes_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines()}
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None and name in exported
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6  # additions only
    assert re.search(r"#define HH_SOBOL_MAX_DIMS 4096\b", hdr) and _ffi.HH_SOBOL_MAX_DIMS == sc.MAX_DIMS == 4096
    assert re.search(r"HH_SOBOL_INCREMENTAL = 0,\s*HH_SOBOL_BRIDGE = 1\b", hdr)
    assert (_ffi.HH_SOBOL_INCREMENTAL, _ffi.HH_SOBOL_BRIDGE) == (sc.INCREMENTAL, sc.BRIDGE) == (0, 1)
    assert "hh_sobol.hip" in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "kDomSobol = 7u" in open(os.path.join(CSRC, "hh_rng.h")).read() and sc.DOM_SOBOL == 7
    assert "#include <hip" not in open(os.path.join(CSRC, "hh_sobol.h")).read()  # a host program includes it


# ---- the direction numbers -----------------------------------------------------------------------------------------------

def test_directions_give_pytorchs_unscrambled_points():
    """hh_sobol_directions for all 4096 dimensions, run through the point rule in numpy for points 0 … 1023, equals
    torch.quasirandom.SobolEngine(4096, scramble=False).draw(1024)·2^32 exactly"""
    torch = pytest.importorskip("torch")
    x = sc.points(sc.directions(range(sc.MAX_DIMS)), np.arange(1024, dtype=np.uint64))
    want = torch.quasirandom.SobolEngine(sc.MAX_DIMS, scramble=False).draw(1024, dtype=torch.float64).numpy() * 2.0 ** 32
    np.testing.assert_array_equal(x.T.astype(np.float64), want)
    v0 = sc.directions([0])[0]
    assert [int(t) for t in v0] == [1 << (31 - j) for j in range(32)]  # dimension 0: van der Corput


def test_directions_refuse_what_the_table_does_not_hold():
    lib, v = _ffi.load_library(), (C.c_uint32 * 32)()
    assert lib.hh_sobol_directions(sc.MAX_DIMS - 1, v) == _ffi.HH_OK and v[0] == 1 << 31
    assert lib.hh_sobol_directions(sc.MAX_DIMS, v) == _ffi.HH_ERR_INVALID
    assert lib.hh_sobol_directions(2 ** 32 - 1, v) == _ffi.HH_ERR_INVALID
    assert lib.hh_sobol_directions(0, None) == _ffi.HH_ERR_INVALID


def test_committed_table_is_what_its_maker_writes():
    """tools/make_sobol_table.py renders scipy's Joe–Kuo file to the committed header, byte for byte: polynomials and
    initial values only, the notice carried, smaller than the largest golden file; and the restated expansion of those
    numbers is the library's, for every dimension"""
    pytest.importorskip("scipy")
    maker = _load("tools/make_sobol_table.py", "make_sobol_table")
    text = open(maker.OUT).read()
    assert text == maker.render()
    assert "Copyright (c) 2008, Frances Y. Kuo and Stephen Joe" in text and "Redistributions of source code must retain" in text
    golden = os.path.join(ROOT, "tests", "golden")
    assert len(text) <= max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden)
                            if os.path.isfile(os.path.join(golden, f)))
    poly, m = maker.load()
    v = sc.directions(range(sc.MAX_DIMS))
    for d in range(sc.MAX_DIMS):
        assert sc.expand(poly[d], m[d]) == [int(t) for t in v[d]], d


# ---- the bridge table ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sc.BRIDGE_STEPS)
def test_bridge_table(n):
    """every time index is built exactly once, parents before children, and the linear map A from the normals to W has
    A·Aᵀ = min(i, j) to 1e-13; the kernel's walk of the table writes every step once, in ascending order, from slots that
    hold what the table says, within ⌈log2 n⌉ + 2 slots"""
    nodes = sc.bridge_nodes(n)
    assert sorted(nd[1] for nd in nodes) == list(range(1, n + 1))
    built = {0}
    for j, (l, m, r, depth, wl, wr, sd) in enumerate(nodes):
        if j:
            assert l in built and r in built and l < m < r and m == (l + r) // 2 and r - l >= 2
            assert wl + wr == pytest.approx(1.0, abs=1e-15) and sd > 0.0
        else:
            assert (l, m, r, wl, wr, sd) == (0, n, n, 0.0, 0.0, math.sqrt(n))
        built.add(m)
    A = sc.bridge_matrix(n)
    t = np.arange(n + 1)
    assert np.abs(A @ A.T - np.minimum.outer(t, t)).max() <= 1e-13
    ops, n_slots = sc.bridge_ops(n)
    assert len(ops) == 2 * n and n_slots <= math.ceil(math.log2(n)) + 2 if n > 1 else n_slots == 2
    z = np.random.default_rng(n).standard_normal(n)
    d, written = sc.walk(ops, n_slots, list(z))
    assert written == list(range(n))
    np.testing.assert_allclose([d[k] for k in range(n)], np.diff(A @ z), rtol=0, atol=1e-13 * math.sqrt(n))


# ---- csrc/hh_sobol.h as a host program -----------------------------------------------------------------------------------

HOST_DIMS = (0, 1, 2, 3, 7, 503, 1110, 1111, 4095)
HOST_POINTS = (0, 1, 2, 3, 255, 256, 257, 1023, 2 ** 20 - 3, 2 ** 31, 2 ** 32 - 513, 2 ** 32 - 1)
HOST_WORDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x12345678)
HOST_STEPS = sc.BRIDGE_STEPS + (7, 100, 4096)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_host_program(tmp_path, build):
    """tests/c/sobol_host_check.cpp — its own main, csrc/hh_sobol.h included — expands dimensions, evaluates points, forms u
    and tabulates bridges: every number is the Python restatement's, bit for bit, and inside the program the walk of every
    bridge gives the steps its nodes give.  Built plainly and with -fsanitize=address,undefined, and run as a program:
    nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = str(tmp_path / ("sobol_host_check_" + build))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "sobol_host_check.cpp"), "-o", exe], check=True)
    queries = [f"dir {d}" for d in range(sc.MAX_DIMS)] + [f"pt {d} {i}" for d in HOST_DIMS for i in HOST_POINTS] + \
        [f"u {x:x}" for x in HOST_WORDS] + [f"bridge {n}" for n in HOST_STEPS]
    (tmp_path / "queries.txt").write_text("\n".join(queries) + "\n")
    run = subprocess.run([exe, str(tmp_path / "queries.txt")], capture_output=True, text=True, env=host_env(), timeout=300)
    assert run.returncode == 0, run.stderr
    out = {}
    for ln in run.stdout.splitlines():
        out.setdefault(ln.split()[0], []).append(ln.split()[1:])
    v = sc.directions(range(sc.MAX_DIMS))
    assert [[int(t, 16) for t in row[1:]] for row in out["dir"]] == [[int(t) for t in row] for row in v]
    want = sc.points(v[list(HOST_DIMS)], np.array(HOST_POINTS, dtype=np.uint64))
    assert [(int(d), int(i), int(x, 16)) for d, i, x in out["pt"]] == \
        [(d, i, int(want[a, b])) for a, d in enumerate(HOST_DIMS) for b, i in enumerate(HOST_POINTS)]
    assert [(int(x, 16), float.fromhex(u)) for x, u in out["u"]] == [(x, float(sc.u_of(x))) for x in HOST_WORDS]
    assert all(0.0 < float.fromhex(u) < 1.0 for _, u in out["u"])
    nodes = [(int(n), int(j), int(l), int(m), int(r), int(dep), float.fromhex(wl), float.fromhex(wr), float.fromhex(sd))
             for n, j, l, m, r, dep, wl, wr, sd in out["node"]]
    assert nodes == [(n, j, *nd) for n in HOST_STEPS for j, nd in enumerate(sc.bridge_nodes(n))]
    ops = [(int(n), int(t), *(int(k) for k in row[:5]), *(float.fromhex(k) for k in row[5:])) for n, t, *row in out["op"]]
    assert ops == [(n, t, *op) for n in HOST_STEPS for t, op in enumerate(sc.bridge_ops(n)[0])]
    assert [(int(n), int(k)) for n, k in out["slots"]] == [(n, sc.bridge_ops(n)[1]) for n in HOST_STEPS]


def test_make_target_runs_the_host_program_under_the_sanitizers():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"pytest tests/test_sobol_host\.py .*-k host_program", mk)


# ---- the golden file -------------------------------------------------------------------------------------------------------

def test_golden_margins_and_the_makers_first_condition():
    """the recorded ratios clear conditions (c) and (d) of tests/test_gpu_sobol.py by the margin; the maker's 16-step part
    runs again here (the 64-step part takes ten seconds: `python tests/golden/make_sobol_exact.py`)"""
    pytest.importorskip("scipy")
    doc = sc.load_golden()
    assert (doc["seed"], doc["points"], doc["randomizations"], doc["margin"]) == \
        (sc.CONV_SEED, sc.CONV_N_HESTON, sc.CONV_R, sc.CONV_MARGIN) and doc["model"] == sc.HESTON
    assert doc["steps16"]["ratio"] <= 0.5 / sc.CONV_MARGIN
    assert doc["steps64"]["bridge"] * sc.CONV_MARGIN <= doc["steps64"]["incremental"]
    maker = _load("tests/golden/make_sobol_exact.py", "make_sobol_exact")
    est, sd = maker.heston_rqmc(16, sc.BRIDGE)
    mean, se = sc.rqmc(est)
    assert (mean, se) == (doc["steps16"]["price"], doc["steps16"]["std_error"])
    assert sd / math.sqrt(sc.CONV_R * sc.CONV_N_HESTON) == doc["steps16"]["pseudo_random_std_error"]


def test_numpy_philox_is_the_oracles(oracle):
    key = [sc.SHIFT_SEED & 0xFFFFFFFF, sc.SHIFT_SEED >> 32]
    for r in (0, 5, 2 ** 32 - 1):
        got = sc.shift_words(np.arange(16), r, sc.SHIFT_SEED)
        assert [int(t) for t in got] == [int(oracle.philox([d >> 2, r, 0, sc.DOM_SOBOL], key)[d & 3]) for d in range(16)]


# ---- the Python layer ------------------------------------------------------------------------------------------------------

def vanilla(style=None, underlying=None):
    return hh.VanillaOption(100.0, EXP, style or hh.European(), hh.Call(), underlying or hh.Spot())


def test_config_and_summary():
    cfg = hh.SobolConfig(1024)
    assert (cfg.points, cfg.steps, cfg.randomizations, cfg.construction) == (1024, 1, 16, hh.BrownianBridge())
    assert 0 <= cfg.seed < 2 ** 64 and hh.SobolConfig(8, seed=5).seed == 5 and hh.BrownianBridge() != hh.Incremental()
    for bad in (dict(points=0), dict(points=2 ** 32), dict(points=8, steps=0), dict(points=8, randomizations=0),
                dict(points=8, construction="bridge")):
        with pytest.raises(ValueError, match="SobolConfig"):
            hh.SobolConfig(**bad)
    price, se = qmc.summarize([3.0])
    assert price == 3.0 and math.isnan(se)  # R = 1: no standard error
    price, se = qmc.summarize([1.0, 3.0])
    assert price == 2.0 and se == pytest.approx(1.0)  # R = 2: sd = sqrt(2), over sqrt(2)
    price, se = qmc.summarize([hh.Dual(1.0, (0.5,)), hh.Dual(3.0, (1.5,))])
    assert (price.value, price.partials, se) == (2.0, (1.0,), pytest.approx(1.0))
    assert "QuasiMonteCarlo" in hh.solve.__doc__


def test_method_errors_name_what_is_supported():
    bs = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    hi = hh.HestonInputs(REF, 0.03, 100.0, 0.04, 1.5, 0.04, 0.5, -0.7)
    cfg = hh.SobolConfig(8, steps=4, seed=1)
    q = lambda dyn, strat, **kw: hh.QuasiMonteCarlo(dyn, strat, cfg, **kw)  # noqa: E731
    euler_h, euler_g = q(hh.HestonDynamics(), hh.EulerMaruyama()), q(hh.LognormalDynamics(), hh.EulerMaruyama())
    refused = [
        (vanilla(), hi, q(hh.HestonDynamics(), hh.HestonBroadieKaya())),          # its REPLAY draws are not normals
        (vanilla(), hi, q(hh.HestonDynamics(), hh.HestonQE())),
        (vanilla(), hi, q(hh.HestonDynamics(), hh.BlackScholesExact())),
        (vanilla(), bs, q(hh.MertonDynamics(), hh.MertonExact())),
        (vanilla(), bs, q(hh.BatesDynamics(), hh.HestonQE())),
        (vanilla(), bs, q(hh.MultiAssetDynamics(), hh.EulerMaruyama())),
        (vanilla(), bs, q(hh.LocalVolDynamics(), hh.EulerMaruyama())),
        (vanilla(), bs, euler_h), (vanilla(), hi, euler_g),                        # dynamics and inputs must agree
        (hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2)), hi, euler_h),
        (hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.ContinuousMonitoring()), hi, euler_h),
        (hh.DigitalOption(101.0, EXP, hh.Put()), bs, euler_g),
        (hh.LookbackOption(EXP, hh.Call(), monitoring=hh.Monitoring(2)), bs, euler_g),
        (vanilla(style=hh.American()), bs, euler_g),                                # LSM draws its own paths
        (vanilla(underlying=hh.Forward()), bs, euler_g),
        (vanilla(), hi, q(hh.HestonDynamics(), hh.EulerMaruyama(), devices=(0,))),
        (vanilla(), bs, hh.QuasiMonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(8, steps=4))),
    ]
    for payoff, mkt, method in refused:
        with pytest.raises(hh.MethodError, match=r"\(LognormalDynamics, BlackScholesExact\).*\(HestonDynamics, EulerMaruyama\)"):
            hh.solve(hh.PricingProblem(payoff, mkt), method)
    with pytest.raises(hh.MethodError, match="LSM"):
        hh.solve(hh.PricingProblem(vanilla(style=hh.American()), bs), euler_g)
    with pytest.raises(hh.MethodError, match="devices"):
        hh.solve(hh.PricingProblem(vanilla(), hi), q(hh.HestonDynamics(), hh.EulerMaruyama(), devices=(0, 1)))
    with pytest.raises(hh.MethodError, match="many-strike"):
        hh.solve(hh.BasketPricingProblem([vanilla(), vanilla()], bs), euler_g)
    with pytest.raises(hh.MethodError):  # no replay= either: the method fills its own buffer
        hh.solve(hh.PricingProblem(vanilla(), bs), euler_g, replay=np.zeros(8))
    # what MonteCarlo refuses stays refused: a QuasiMonteCarlo is not a MonteCarlo
    assert not isinstance(euler_g, hh.MonteCarlo)
