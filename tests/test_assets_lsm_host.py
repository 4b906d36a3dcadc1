"""American exercise on several assets on the host side, without a GPU: the entry points declared, exported and bound; the
basis of csrc/hh_lsm_basis.h — its count, its order and its φ for every (m, p) — through a stand-alone program, built
plainly and with -fsanitize=address,undefined and run as a program (nothing preloaded, nothing loaded into this
interpreter); the host routing, every MethodError, and simulate_asset_paths' shapes against a fake library."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import assets_cases as ac
from tests import assets_lsm_cases as A
from tests.conftest import host_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_assets_path_rows": 8, "hh_lsm_solve_states": 11, "hh_lsm_solve_assets": 11}
REF, EXP = hh.Date(2025, 1, 1), hh.Date(2026, 1, 1)


def test_new_prototypes_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines()}
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto and len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None and name in exported
    assert re.search(r"\bsize_t\s+hh_assets_rows_elems\s*\(", hdr) and "hh_assets_rows_elems" in exported
    assert lib.hh_assets_rows_elems(513, 12, 3, 1) == 13 * 3 * 1026
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    assert re.search(r"#define HH_LSM_MAX_BASIS 45\b", hdr) and _ffi.HH_LSM_MAX_BASIS == 45
    assert C.sizeof(_ffi.hh_lsm_states) == 32 + 8 * _ffi.HH_MAX_ASSETS and _ffi.hh_lsm_states.weights.offset == 32
    assert '"hh_lsm_multi.hip"' in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "#include <hip" not in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_lsm_basis.h")).read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_basis_host_program(tmp_path, build):
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = tmp_path / ("lsm_basis_check_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "lsm_basis_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=host_env(), timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    seen = set()
    for line in lines[:90]:
        head, _, tail = line.partition("|")
        m, p, B, *words = head.split()
        m, p, B = int(m), int(p), int(B)
        seen.add((m, p))
        admitted = 1 <= m <= 8 and 1 <= p <= 8 and math.comb(m + p, p) <= 45
        assert B == (math.comb(m + p, p) if admitted else 0), (m, p)
        assert (p <= A.ADMITTED.get(m, 0) and p >= 1) == admitted
        if not admitted:
            assert not words and not tail.split()
            continue
        expo = A.basis(m, p)
        assert [int(w, 16) for w in words] == A.basis_words(m, p)
        # graded: the degrees never fall; within a degree the tuples fall lexicographically; all distinct; B of them
        assert [sum(t) for t in expo] == sorted(sum(t) for t in expo) and len(set(expo)) == B
        assert all(a > b for a, b in zip(expo, expo[1:]) if sum(a) == sum(b))
        assert expo[0] == (0,) * m and expo[1:m + 1] == [tuple(int(i == k) for i in range(m)) for k in range(m)]
        z = np.array([[(i + 2) / 8.0 - 1.0] for i in range(m)])
        assert [float.fromhex(t) for t in tail.split()] == list(A.phi(z, expo)[:, 0])
    assert seen == {(m, p) for m in range(1, 10) for p in range(10)}
    assert lines[90].split() == ["padding", "0x0p+0", "0x0p+0"]
    assert [tuple(map(int, t.split()[1:])) for t in lines[91:]] == sorted(A.ADMITTED.items())


# ---- the host's routes against a fake library ----------------------------------------------------------------------------------

class FakeLib:
    def __init__(self):
        self.calls = []

    def hh_lsm_solve_assets(self, handle, model, assets, cfg, every, degree, discount, res, tau, val, rows):
        m, a, c = model._obj, assets._obj, cfg._obj
        self.calls.append(dict(entry="hh_lsm_solve_assets", every=every, degree=degree, discount=discount, kind=a.index_kind,
                               d=a.n_assets, weights=list(a.weights[:a.n_assets]), strike=m.strike, cp=m.cp, T=m.T, r=m.r_drift,
                               n=c.n_paths, steps=c.n_steps, anti=c.antithetic, outs=(tau, val, rows)))
        if rows:
            C.memset(rows, 0, 8 * (c.n_steps // every + 1) * a.n_assets * c.n_paths * (2 if c.antithetic else 1))
        res._obj.price, res._obj.std_error = 12.5, 0.03
        return 0

    def hh_assets_path_rows(self, handle, model, assets, cfg, every, rows, on_device, res):
        a, c = assets._obj, cfg._obj
        n = c.n_paths * (2 if c.antithetic else 1)
        shape = (c.n_steps // every + 1, a.n_assets, n)
        out = np.ctypeslib.as_array(C.cast(rows, C.POINTER(C.c_double)), shape=(int(np.prod(shape)),)).reshape(shape)
        out[:] = np.log(2.0)
        self.calls.append(dict(entry="hh_assets_path_rows", every=every, shape=shape, on_device=on_device))
        return 0


class FakeCtx:
    handle = None

    def __init__(self):
        self.lib = FakeLib()

    def check(self, rc):
        assert rc == 0


@pytest.fixture
def fake(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(_ffi, "get_context", lambda device=0: ctx)
    return ctx.lib


def _inputs(case=ac.CASE_B, **kw):
    return hh.MultiAssetInputs(REF, kw.get("rate", case["r_drift"]), kw.get("spots", case["spots"]), case["sigmas"], case["corr"])


def _lsm(degree=3, steps=12, n=16, vr=None, **kw):
    cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(n), variance_reduction=vr)
    return hh.LSM(hh.MonteCarlo(hh.MultiAssetDynamics(), hh.EulerMaruyama(), cfg, **kw), degree)


def _american(index=None, K=100.0, cp=None):
    return hh.IndexOption(index or hh.WorstOf(), hh.VanillaOption(K, EXP, hh.American(), cp or hh.Put(), hh.Spot()))


def test_the_solve_route(fake):
    inp = _inputs()
    sol = hh.solve(hh.PricingProblem(_american(), inp), _lsm(), exercise_every=3)
    assert isinstance(sol, hh.LSMSolution) and sol.price == 12.5 and sol.std_error == 0.03
    (call,) = fake.calls
    assert (call["entry"], call["every"], call["degree"], call["kind"], call["d"]) == ("hh_lsm_solve_assets", 3, 3, ac.WORST, 2)
    assert call["weights"] == [1.0, 1.0] and (call["strike"], call["cp"]) == (100.0, -1.0)
    assert (call["n"], call["steps"], call["anti"]) == (16, 12, 0)
    assert call["discount"] == pytest.approx(math.exp(-0.03 * call["T"] * 3 / 12), rel=1e-12)
    assert call["outs"][0] is not None and call["outs"][1] is not None and call["outs"][2] is None
    assert sol.stopping_info[0].shape == (16,) and sol.spot_paths is None
    fake.calls.clear()
    basket = _american(hh.WeightedSum((0.5, 0.5)), 95.0, hh.Call())
    sol = hh.solve(hh.PricingProblem(basket, inp), _lsm(2, vr=hh.Antithetic()), spot_paths=True, stopping_info=False)
    (call,) = fake.calls
    assert (call["kind"], call["weights"], call["cp"], call["every"], call["anti"]) == (ac.SUM, [0.5, 0.5], 1.0, 1, 1)
    assert sol.stopping_info is None and sol.spot_paths.shape == (13, 2, 32)
    fake.calls.clear()
    # plain solves under FiniteDifference: the bumped problems take the same route
    g = hh.solve(hh.GreekProblem(hh.PricingProblem(_american(), inp), hh.AssetSpotLens(0)), hh.FiniteDifference(1e-2), _lsm())
    assert len(fake.calls) >= 2 and {c["entry"] for c in fake.calls} == {"hh_lsm_solve_assets"} and g.greek == 0.0


def test_simulate_asset_paths(fake):
    inp = _inputs(ac.CASE_A)
    prob = hh.PricingProblem(_american(hh.BestOf((1.0, 2.0, 0.5))), inp)
    mc = _lsm(steps=12, n=8, vr=hh.Antithetic()).mc_method
    paths = hh.simulate_asset_paths(prob, mc, exercise_every=4)
    assert paths.spot.shape == (4, 3, 16) and np.all(paths.spot == np.exp(np.log(2.0)))
    assert np.allclose(paths.times, np.linspace(0.0, float(hh.yearfrac(REF, EXP)) if hasattr(hh, "yearfrac") else paths.times[-1], 4))
    assert fake.calls == [dict(entry="hh_assets_path_rows", every=4, shape=(4, 3, 16), on_device=0)]
    assert "w_i·S_i" in hh.simulate_asset_paths.__doc__ and "w_i·S_i" in hh.AssetPaths.__doc__


def test_refusals_touch_no_device(fake):
    inp, prob = _inputs(), hh.PricingProblem(_american(), _inputs())
    mc_plain = _lsm().mc_method
    dual = hh.Dual(100.0, (1.0,))
    cont = hh.IndexOption(hh.WorstOf(), hh.BarrierOption(100.0, 50.0, EXP, hh.Put(), hh.DownAndOut(), monitoring=hh.ContinuousMonitoring()))
    asian = hh.IndexOption(hh.WorstOf(), hh.AsianOption(100.0, EXP, hh.Put()))
    european = hh.IndexOption(hh.WorstOf(), hh.VanillaOption(100.0, EXP, hh.European(), hh.Put(), hh.Spot()))
    wide = hh.MultiAssetInputs(REF, 0.03, *[ac.path_case(8)[k] for k in ("spots", "sigmas", "corr")])
    cases = [
        (prob, mc_plain, {}, "American exercise is not offered on an index of several assets"),   # MonteCarlo keeps its refusal: not through it
        (hh.PricingProblem(_american(), inp.replace(spots=(dual, 95.0))), _lsm(), {}, "FiniteDifference"),
        (hh.PricingProblem(_american(hh.WorstOf((dual, 1.0))), inp), _lsm(), {}, "FiniteDifference"),
        (hh.PricingProblem(_american(K=dual), inp), _lsm(), {}, "FiniteDifference"),
        (prob, _lsm(devices=range(2)), {}, "one device"),
        (hh.PricingProblem(cont, inp), _lsm(), {}, "path-dependent inner payoff"),
        (hh.PricingProblem(asian, inp), _lsm(), {}, "path-dependent inner payoff"),
        (hh.PricingProblem(european, inp), _lsm(), {}, "needs an American VanillaOption on Spot"),
        (hh.PricingProblem(_american(hh.WeightedSum([0.125] * 8)), wide), _lsm(3), {}, "165 basis functions"),
        (prob, _lsm(9), {}, "degree 1 … 8"),
        (prob, _lsm(), dict(exercise_every=5), "must be a whole number >= 1 that divides steps"),
        (prob, _lsm(), dict(exercise_every=0), "must be a whole number >= 1 that divides steps"),
        (prob, _lsm(), dict(path_state="spot"), "path_state applies to the Euler path sources only"),
        (hh.PricingProblem(_american(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)), _lsm(), {}, "multi-asset"),
        (prob, hh.LSM(hh.LognormalDynamics(), hh.BlackScholesExact(), hh.SimulationConfig(8, seeds=np.arange(8)), 3), {}, "multi-asset"),
        (hh.PricingProblem(hh.VanillaOption(100.0, EXP, hh.American(), hh.Put(), hh.Spot()), inp), _lsm(), {}, "IndexOption"),
    ]
    for k, (p, method, kw, words) in enumerate(cases):
        with pytest.raises(hh.MethodError, match=re.escape(words)):
            hh.solve(p, method, **kw)
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.GreekProblem(prob, hh.AssetSpotLens(0)), hh.ForwardAD(), _lsm())
    with pytest.raises(ValueError, match="3 weights for 2 assets"):
        hh.solve(hh.PricingProblem(_american(hh.WorstOf((1.0, 1.0, 1.0))), inp), _lsm())
    with pytest.raises(hh.MethodError, match="divides steps"):
        hh.simulate_asset_paths(prob, mc_plain, exercise_every=7)
    with pytest.raises(hh.MethodError, match="one device"):
        hh.simulate_asset_paths(prob, _lsm(devices=range(2)).mc_method)
    assert fake.calls == []
