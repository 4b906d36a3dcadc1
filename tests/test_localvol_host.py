"""Local volatility on a tabulated surface, everything that needs no GPU: the C-ABI's declarations, the host program on
csrc/hh_localvol.h (tests/c/localvol_host_check.cpp), the restatement of tests/localvol_cases.py itself, Dupire's formula
against the CEV model's closed form (tests/golden/localvol_exact.json), and the Python route with every refusal."""
import ctypes as C
import importlib.util
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from hedgehog_jl_amd import localvol as hlv  # noqa: E402
from tests import localvol_cases as lc  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_lv": 10, "hh_mc_solve_path_lv": 12}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


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
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    assert re.search(r"#define HH_LV_MAX_NODES\s+8192\b", hdr) and _ffi.HH_LV_MAX_NODES == 8192
    assert "hh_localvol.hip" in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "#include <hip" not in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_localvol.h")).read()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_hh_localvol_layout(tmp_path):
    """hh_localvol is 40 bytes — two pointers, two doubles, two uint32: a compiled offsetof dump against ctypes"""
    fields = [n for n, _ in _ffi.hh_localvol._fields_]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(hh_localvol));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(hh_localvol, {f}), sizeof(((hh_localvol*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, env=host_env()).stdout.split("\n")
    assert out[0] == "sizeof 40" and C.sizeof(_ffi.hh_localvol) == 40
    got = [(n, getattr(_ffi.hh_localvol, n).offset, getattr(_ffi.hh_localvol, n).size) for n in fields]
    want = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:1 + len(fields)]]
    assert got == want == [("times", 0, 8), ("vols", 8, 8), ("x_lo", 16, 8), ("h", 24, 8), ("n_times", 32, 4), ("n_x", 36, 4)]
    lv = _ffi.make_localvol([0.5, 1.0], [[0.2, 0.3, 0.4], [0.25, 0.35, 0.45]], 4.0, 0.25)
    assert (lv.n_times, lv.n_x, lv.x_lo, lv.h, lv.vols[5], lv.times[1]) == (2, 3, 4.0, 0.25, 0.45, 1.0)


# ---- the host program ----------------------------------------------------------------------------------------------------

def sweep():
    """[(surface, [(t, x, r, dt, dW)])]: n_times in {1, 2, 5} × n_x in {2, 3, 33}; x below, on and above the grid, on nodes
    and between them; t before, on, between and after the times"""
    rng = np.random.default_rng(20240611)
    out = []
    for n_t in (1, 2, 5):
        for n_x in (2, 3, 33):
            x_lo, h = 4.0 + 0.01 * n_t, (0.1 if n_x == 33 else 0.3) / (n_x - 1) * (1.0 + 0.1 * n_t)
            times = [0.25 + 0.2 * j + 0.01 * j * j for j in range(n_t)]
            vols = rng.uniform(0.1, 0.6, size=(n_t, n_x))
            surf = dict(times=np.array(times), vols=vols, x_lo=x_lo, h=h)
            ts = [0.0, 0.1, times[0], times[-1], times[-1] + 0.3] + [0.5 * (a + b) for a, b in zip(times, times[1:])] + \
                [float(np.nextafter(t, s)) for t in times for s in (0.0, 9.0)]
            xs = [x_lo - 1.0, x_lo, float(np.nextafter(x_lo, 0.0)), x_lo + h * (n_x - 1), x_lo + h * (n_x - 1) + 0.5,
                  float(np.nextafter(x_lo + h * (n_x - 1), 9.0))] + [x_lo + h * i for i in range(n_x)] + \
                [float(x_lo + h * u) for u in rng.uniform(0.0, n_x - 1, size=6)]
            qs = [(t, x, 0.03, 1.0 / 64, float(rng.normal(0.0, 0.125))) for t in ts for x in xs]
            out.append((surf, qs))
    return out


def restated(surf, q):
    t, x, r, dt, dW = q
    times = [float(s) for s in surf["times"]]
    flat = [float(v) for v in surf["vols"].reshape(-1)]
    n_t, n_x = surf["vols"].shape
    j, w = lc.row_of(times, t)
    i, f, where = lc.cell_of(x, float(surf["x_lo"]), 1.0 / float(surf["h"]), n_x)
    sg = lc.sigma_of(flat, n_x, j, w, n_t > 1, i, f)
    return j, w, where, sg, lc.step_of(x, sg, r, dt, dW)


def _build_host_check(tmp_path, flags, name):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "localvol_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_lookup_and_step_host_program(tmp_path, build):
    """tests/c/localvol_host_check.cpp — its own main, csrc/hh_localvol.h included — takes lookup-and-step over the
    sweep: every j, w, σ and x′ is the Python-float restatement's, bit for bit (the same IEEE operations in the same
    order), and inside the program every σ and x′ lies within 1e-13 of a long-double evaluation.  Built plainly and with
    -fsanitize=address,undefined, and run as a program: nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = _build_host_check(tmp_path, flags, "localvol_host_check_" + build)
    cases = sweep()
    with open(tmp_path / "rows.txt", "w") as f:
        for surf, qs in cases:
            n_t, n_x = surf["vols"].shape
            nums = [surf["x_lo"], surf["h"]] + list(surf["times"]) + list(surf["vols"].reshape(-1))
            f.write(f"T {n_t} {n_x} " + " ".join(float(t).hex() for t in nums) + "\n")
            for q in qs:
                f.write("Q " + " ".join(float(t).hex() for t in q) + "\n")
    run = subprocess.run([exe, str(tmp_path / "rows.txt")], capture_output=True, text=True, env=host_env(), timeout=120)
    assert run.returncode == 0, run.stderr
    got = [ln.split() for ln in run.stdout.splitlines()]
    rows = [(surf, q) for surf, qs in cases for q in qs]
    assert len(got) == len(rows)
    seen, weights = set(), set()
    for (surf, q), (j, w, where, sg, xn) in zip(rows, got):
        want = restated(surf, q)
        assert (int(j), float.fromhex(w), int(where), float.fromhex(sg), float.fromhex(xn)) == want, (q, j, w, sg, xn, want)
        seen.add((surf["vols"].shape, want[2]))
        weights.add((surf["vols"].shape[0], 0 if want[1] == 0.0 else 2 if want[1] == 1.0 else 1))
    assert seen == {((n_t, n_x), wh) for n_t in (1, 2, 5) for n_x in (2, 3, 33) for wh in (-1, 0, 1)}
    assert weights == {(1, 0)} | {(n_t, k) for n_t in (2, 5) for k in (0, 1, 2)}  # both time clamps and the interior
    assert re.search(r"compared [1-9]\d* steps; 0 bad", run.stderr), run.stderr


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def test_constant_table_reproduces_the_lognormal_step():
    """fma(·, 0, c) = c: on a table of equal entries σ is that entry whatever t and x, and the step is GbmModel::step's —
    fma(σ, dW, fma(dt, r − (0.5·σ)·σ, x)) — bit for bit"""
    rng = np.random.default_rng(3)
    for s0 in (0.2, 0.3141592653589793, 1e-3):
        surf = dict(times=np.array([0.2, 0.5, 0.9]), vols=np.full((3, 7), s0), x_lo=4.0, h=0.1)
        for _ in range(50):
            t, x, dW = float(rng.uniform(0, 1.2)), float(rng.uniform(3.5, 5.2)), float(rng.normal(0, 0.1))
            assert lc.get_sigma(surf, t, x) == s0
            g = 0.03 - 0.5 * s0 * s0
            assert lc.step_of(x, s0, 0.03, 1 / 64, dW) == lc.fma(s0, dW, lc.fma(1 / 64, g, x))


def test_lookup_is_continuous_across_cell_edges_and_clamps():
    """one ulp either side of a node, of either end of the grid and of a time: σ moves by a few ulps"""
    surf = lc.surface("narrow")
    n_x = surf["vols"].shape[1]
    for i in range(n_x):
        x = surf["x_lo"] + surf["h"] * i
        for t in (0.0, 0.2, 0.275, 0.5, 0.8, 1.0):
            lo, mid, hi = (lc.get_sigma(surf, t, float(y)) for y in (np.nextafter(x, 0.0), x, np.nextafter(x, 9.0)))
            assert abs(lo - mid) <= 8 * np.spacing(mid) and abs(hi - mid) <= 8 * np.spacing(mid), (i, t, lo, mid, hi)
    for t in surf["times"]:
        lo, mid, hi = (lc.get_sigma(surf, float(s), lc.X0 + 0.0123) for s in (np.nextafter(t, 0.0), t, np.nextafter(t, 9.0)))
        assert abs(lo - mid) <= 8 * np.spacing(mid) and abs(hi - mid) <= 8 * np.spacing(mid), (t, lo, mid, hi)


def test_python_surface_evaluates_the_same_lookup():
    surf = lc.surface("narrow")
    s = hh.LocalVolSurface(surf["times"], surf["x_lo"] + surf["h"] * np.arange(33), surf["vols"])
    rng = np.random.default_rng(5)
    for _ in range(100):
        t, x = float(rng.uniform(0, 1)), float(rng.uniform(lc.X0 - 0.12, lc.X0 + 0.12))
        S = math.exp(x)
        assert hh.get_local_vol(s, t, S) == lc.get_sigma(dict(surf, x_lo=s.x_lo, h=s.h), t, math.log(S))
    with pytest.raises(ValueError, match="uniform"):
        hh.LocalVolSurface([0.5], [4.0, 4.1, 4.25], [[0.2, 0.2, 0.2]])
    with pytest.raises(ValueError, match="strictly increasing"):
        hh.LocalVolSurface([0.5, 0.5], [4.0, 4.1], [[0.2, 0.2], [0.2, 0.2]])
    with pytest.raises(ValueError, match="> 0"):
        hh.LocalVolSurface([0.5], [4.0, 4.1], [[0.2, 0.0]])
    with pytest.raises(ValueError, match="HH_LV_MAX_NODES"):
        hh.LocalVolSurface(np.arange(1, 34) * 0.01, np.arange(256) * 0.01, np.full((33, 256), 0.2))
    flat = hh.LocalVolSurface.sample(lambda t, S: 0.2 + 0.001 * t, [0.1, 0.9], 4.0, 5.0, 11)
    assert flat.vols.shape == (2, 11) and flat.vols[1, 3] == 0.2 + 0.001 * 0.9


# ---- Dupire against the CEV model ---------------------------------------------------------------------------------------

def test_fixture_conditions_and_its_maker():
    """the fixture is what tests/golden/make_localvol_exact.py says it writes: the model, the grids, the centre nodes of
    the coarse grid, and — recomputed here for a handful of stencil points — its prices"""
    doc = lc.load_golden()
    spec = importlib.util.spec_from_file_location("make_lv", os.path.join(ROOT, "tests", "golden", "make_localvol_exact.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    times, xs = mk.nodes()
    assert doc["model"] == lc.CEV and doc["times"] == times and (doc["x_lo"], doc["x_hi"], doc["n_x"]) == (xs[0], xs[-1], 257)
    assert doc["grids"] == {"coarse": dict(dk=0.02, dT=0.01), "fine": dict(dk=0.01, dT=0.005)}
    centre = [[j, i] for j, t in enumerate(times) for i, x in enumerate(xs) if mk.centre(t, x)]
    assert doc["coarse_nodes"] == centre and doc["coarse"].shape == (len(centre), 5) and doc["coarse"].dtype == np.float64
    fine = doc["fine"]
    assert fine.shape == (5, 21, 257) and fine.dtype == np.float64 and np.all(np.isfinite(fine)) and np.all(np.isfinite(doc["coarse"]))
    for j, i in ((0, 128), (20, 0), (10, 256), (3, 100)):
        for s, tk in enumerate(mk.stencil(times[j], xs[i], 0.01, 0.005)):
            assert mk.price(tk) == fine[s, j, i], (j, i, s)
    j, i = doc["coarse_nodes"][17]
    assert [mk.price(tk) for tk in mk.stencil(times[j], xs[i], 0.02, 0.01)] == list(doc["coarse"][17])


def test_dupire_recovers_the_cev_local_volatility_at_second_order():
    """σ² = 2(C_T + rC_k)/(C_kk − C_k) by central differences on exact CEV prices, over the nodes with
    |x − log S0| <= 2.5·0.25·√t: every node is valid, and halving dk and dT divides the largest relative error against
    σ0(S/S0)^{β−1} by a factor in [3, 5] — central differences are of second order, so the factor is 4 up to the next
    term of the expansion; nothing here is fitted.
    Measured: coarse (dk = 0.02, dT = 0.01) and fine (0.01, 0.005) errors are printed (`-s`)."""
    doc = lc.load_golden()
    times, x = np.array(doc["times"]), doc["x_lo"] + (doc["x_hi"] - doc["x_lo"]) / 256 * np.arange(257)
    S0, r = lc.CEV["S0"], lc.CEV["r"]
    true = lc.cev_sigma(np.exp(x))
    fine_sig, fine_ok = hlv.dupire_from_stencil(np.array(doc["fine"]), r, 0.01, 0.005, S0)
    jj, ii = np.array(doc["coarse_nodes"]).T
    coarse_sig, coarse_ok = hlv.dupire_from_stencil(doc["coarse"].T, r, 0.02, 0.01, S0)
    assert coarse_ok.all() and fine_ok[jj, ii].all()
    e_coarse = np.max(np.abs(coarse_sig / true[ii] - 1.0))
    e_fine = np.max(np.abs(fine_sig[jj, ii] / true[ii] - 1.0))
    print(f"Dupire on CEV: largest relative error coarse {e_coarse:.3e}, fine {e_fine:.3e}, ratio {e_coarse / e_fine:.2f}")
    assert 3.0 <= e_coarse / e_fine <= 5.0, (e_coarse, e_fine)
    # the surface dupire_local_vol makes of the fine grid: the same numbers where valid, the neighbour's elsewhere, clamped
    surf, valid = hlv.dupire_local_vol(lambda T, K: np.array(doc["fine"]).reshape(-1), times, doc["x_lo"], doc["x_hi"], 257, r,
                                       0.01, 0.005, vol_bounds=(0.02, 1.5), spot=S0, return_valid=True)
    assert np.array_equal(valid, fine_ok) and np.array_equal(surf.vols[valid], np.clip(fine_sig[valid], 0.02, 1.5))
    assert surf.vols.min() >= 0.02 and surf.vols.max() <= 1.5
    for j in range(21):
        bad = np.flatnonzero(~valid[j])
        for i in bad:
            toward = i - 1 if i > 128 else i + 1
            assert surf.vols[j, i] == surf.vols[j, toward]


# ---- the Python route and every refusal ----------------------------------------------------------------------------------

def _inputs():
    s = hh.LocalVolSurface.sample(lambda t, S: 0.25 * (S / 100.0) ** -0.5, [0.1, 0.5], lc.X0 - 1.0, lc.X0 + 1.0, 33)
    return hh.LocalVolInputs(REF, 0.03, 100.0, s)


def _mc(dynamics=None, strategy=None, **kw):
    return hh.MonteCarlo(dynamics or hh.LocalVolDynamics(), strategy or hh.EulerMaruyama(),
                         hh.SimulationConfig(256, steps=4, seeds=np.arange(1, 257, dtype=np.uint64)), **kw)


def test_python_refusals_name_the_route():
    m = _inputs()
    call = hh.VanillaOption(100.0, EXP, hh.European(), hh.Call(), hh.Spot())
    prob = hh.PricingProblem(call, m)
    with pytest.raises(hh.MethodError, match=re.escape(hlv.ROUTES)):
        hh.solve(prob, _mc(strategy=hh.BlackScholesExact()))
    with pytest.raises(hh.MethodError, match=re.escape(hlv.ROUTES)):
        hh.solve(prob, _mc(dynamics=hh.LognormalDynamics()))
    bs = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    with pytest.raises(hh.MethodError, match=re.escape(hlv.ROUTES)):
        hh.solve(hh.PricingProblem(call, bs), _mc())
    with pytest.raises(hh.MethodError, match="American exercise is not offered on local-volatility paths"):
        hh.solve(hh.PricingProblem(hh.VanillaOption(100.0, EXP, hh.American(), hh.Put(), hh.Spot()), m), _mc())
    for method in (hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics()), hh.BlackScholesAnalytic(), hh.CoxRossRubinsteinMethod(16),
                   hh.CrankNicolsonMethod(64, 16)):
        with pytest.raises(hh.MethodError, match=f"{type(method).__name__} does not price local volatility: use " + re.escape(hlv.ROUTES)):
            hh.solve(prob, method)
        with pytest.raises(hh.MethodError, match="does not price local volatility"):
            hh.solve(hh.BasketPricingProblem([call], m), method)
    with pytest.raises(hh.MethodError, match=r"no dual partials \(ForwardAD\)"):
        hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.ForwardAD(), _mc())
    with pytest.raises(hh.MethodError, match="one device"):
        hh.solve(prob, _mc(devices=(0, 1)))
    # the lenses FiniteDifference moves: the spot and the curve move, the surface stays
    bumped = hh.set(prob, hh.SpotLens(), 101.0)
    assert bumped.market_inputs.spot == 101.0 and bumped.market_inputs.surface is m.surface
    assert hh.ZeroRateSpineLens(1)(prob) == 0.03
    assert hh.set(prob, hh.ZeroRateSpineLens(1), 0.04).market_inputs.surface is m.surface
