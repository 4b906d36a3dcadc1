"""hh_mc_path_grid and hh_lsm_solve_path on the host side, without a GPU: hh_path_source packed as the header lays it out;
the two prototypes declared, exported and bound, the ABI still 6; the new solve forms reach hh_lsm_solve_path with the
route's structs and the discount of one exercise period; what the host refuses, it refuses before any device is touched;
the refusals that were pinned before stay as they are."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from hedgehog_jl_amd import lsm as hlsm
from hedgehog_jl_amd import routes
from tests.conftest import host_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_grid": 8, "hh_lsm_solve_path": 11}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
KINDS = ("HH_SOURCE_EULER", "HH_SOURCE_JUMP", "HH_SOURCE_QE", "HH_SOURCE_BATES", "HH_SOURCE_LOCALVOL", "HH_SOURCE_VG")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_hh_path_source_layout(tmp_path):
    """a compiled offsetof dump against the ctypes structure, and the enum's values"""
    fields = [n for n, _ in _ffi.hh_path_source._fields_]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(hh_path_source));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(hh_path_source, {f}), sizeof(((hh_path_source*)0)->{f}));' for f in fields]
    lines += [f'  printf("{k} %d\\n", (int){k});' for k in KINDS]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, env=host_env()).stdout.split("\n")
    assert out[0] == f"sizeof {C.sizeof(_ffi.hh_path_source)}" == "sizeof 40"
    got = [(n, getattr(_ffi.hh_path_source, n).offset, getattr(_ffi.hh_path_source, n).size) for n in fields]
    want = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:1 + len(fields)]]
    assert got == want == [("kind", 0, 4), ("jump", 8, 8), ("qe", 16, 8), ("localvol", 24, 8), ("vg", 32, 8)]
    for k, ln in zip(KINDS, out[1 + len(fields):]):
        assert ln == f"{k} {getattr(_ffi, k)}"
    j, g = _ffi.make_jump(0.8, -0.1, 0.15), _ffi.make_vg(-0.3, 0.5)
    src = _ffi.make_path_source(_ffi.HH_SOURCE_JUMP, jump=j)
    assert src.kind == 1 and src.jump.contents.mu_j == -0.1 and not src.qe and not src.localvol and not src.vg
    assert _ffi.make_path_source(_ffi.HH_SOURCE_VG, vg=g).vg.contents.nu == 0.5


def test_new_prototypes_are_declared_exported_and_bound():
    raw = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
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
    assert re.search(r"#define HH_ABI_VERSION 6\b", raw)
    assert re.search(r"enum hh_path_source_kind \{ HH_SOURCE_EULER = 0, HH_SOURCE_JUMP = 1, HH_SOURCE_QE = 2, HH_SOURCE_BATES = 3,", hdr)
    # the doc block says what the rows are, whose trajectories they are and what is not provided
    for text in ("row 0   S0 in every column", "after step j·exercise_every", "on the same seeds", "date_discount is the discount over ONE EXERCISE PERIOD",
                 "EXERCISE DATES", "Not provided: sharded and multi-GPU forms, the log path state", "variance rows for QE and Bates"):
        assert text in raw, text


# ---- the host route -------------------------------------------------------------------------------------------------------

def put(style=None, K=100.0):
    return hh.VanillaOption(K, EXP, style or hh.American(), hh.Put(), hh.Spot())


def config(n=8, steps=12, **kw):
    return hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64), **kw)


def surface():
    x = np.log(100.0) - 1.0 + 2.0 / 64 * np.arange(65)
    return hh.LocalVolSurface([0.25, 0.75], x, np.full((2, 65), 0.2))


CURVE = hh.RateCurve(REF, [0.5, 2.0], zeros=[0.01, 0.04])
MARKETS = {
    "merton": lambda r=0.03, S=100.0: hh.MertonInputs(REF, r, S, 0.2, 0.8, -0.1, 0.15),
    "qe": lambda r=0.03, S=100.0: hh.HestonInputs(REF, r, S, 0.04, 2.0, 0.04, 0.3, -0.7),
    "bates": lambda r=0.03, S=100.0: hh.BatesInputs(REF, r, S, 0.04, 2.0, 0.04, 0.3, -0.7, 0.8, -0.1, 0.15),
    "localvol": lambda r=0.03, S=100.0: hh.LocalVolInputs(REF, r, S, surface()),
    "vg": lambda r=0.03, S=100.0: hh.VarianceGammaInputs(REF, r, S, 0.2, -0.3, 0.5),
}
PAIRS = {
    "merton": (hh.MertonDynamics, hh.EulerMaruyama, _ffi.HH_SOURCE_JUMP, ("jump",)),
    "qe": (hh.HestonDynamics, lambda: hh.HestonQE(1.5, True), _ffi.HH_SOURCE_QE, ("qe",)),
    "bates": (hh.BatesDynamics, lambda: hh.HestonQE(1.5, True), _ffi.HH_SOURCE_BATES, ("qe", "jump")),
    "localvol": (hh.LocalVolDynamics, hh.EulerMaruyama, _ffi.HH_SOURCE_LOCALVOL, ("localvol",)),
    "vg": (hh.VarianceGammaDynamics, hh.VarianceGammaExact, _ffi.HH_SOURCE_VG, ("vg",)),
}


def lsm_of(name, cfg=None, degree=3, **kw):
    dyn, strat, _, _ = PAIRS[name]
    return hh.LSM(hh.MonteCarlo(dyn(), strat(), cfg or config(), **kw), degree)


class FakeLib:
    """records the one call an LSM solve makes and answers it as a solve would"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class FakeContext:
    handle = None

    def __init__(self):
        self.lib = FakeLib()

    def check(self, rc):
        assert rc == 0


@pytest.fixture
def fake(monkeypatch):
    ctx = FakeContext()
    monkeypatch.setattr(_ffi, "get_context", lambda device=0: ctx)
    return ctx


def _deref(byref_obj):
    return byref_obj._obj


@pytest.mark.parametrize("every", [1, 3, 12])
@pytest.mark.parametrize("name", list(PAIRS))
def test_solve_reaches_hh_lsm_solve_path_with_the_discount_of_one_exercise_period(fake, name, every):
    mkt = MARKETS[name](r=CURVE)
    cfg = config(8, 12, variance_reduction=hh.Antithetic())
    sol = hh.solve(hh.PricingProblem(put(K=95.0), mkt), lsm_of(name, cfg, degree=4), exercise_every=every, spot_paths=True)
    (entry, args), = fake.lib.calls
    assert entry == "hh_lsm_solve_path"
    _, source, model, c, ex, degree, D, _, tau, val, grid = args
    source, model, c = _deref(source), _deref(model), _deref(c)
    _, _, kind, fields = PAIRS[name]
    assert source.kind == kind
    for f in ("jump", "qe", "localvol", "vg"):
        assert bool(getattr(source, f)) == (f in fields), (name, f)
    T = hh.yearfrac(REF, EXP)
    assert (ex, degree) == (every, 4) and model.T == T
    assert D == float(hh.df(mkt.rate, mkt.referenceDate + (T * every / 12) * hlsm.MILLISECONDS_IN_YEAR_365))
    assert D == pytest.approx(float(hh.df(mkt.rate, EXP)) if every == 12 else D) and 0.9 < D < 1.0
    if every < 12:  # … and under a flat rate: exp(−r·T·exercise_every/steps)
        fake.lib.calls.clear()
        hh.solve(hh.PricingProblem(put(), MARKETS[name](r=0.05)), lsm_of(name, cfg), exercise_every=every)
        assert fake.lib.calls[0][1][6] == pytest.approx(np.exp(-0.05 * T * every / 12), rel=1e-12)
    assert (model.strike, model.cp, model.S0) == (95.0, -1.0, 100.0)
    assert (c.n_paths, c.n_steps, c.antithetic, c.n_partials, c.seeds_on_device, c.seeds_len) == (8, 12, 1, 0, 0, 8)
    # the structs are the route's own: those of its path solve to the same expiry
    route = routes.lsm_route_of(mkt, lsm_of(name, cfg).mc_method)
    want_m, want_c, extras = route.form_structs(put(hh.European()), mkt, lsm_of(name, cfg).mc_method)
    assert (c.dynamics, c.strategy, c.em_split) == (want_c.dynamics, want_c.strategy, want_c.em_split)
    assert (model.r_drift, model.sigma, model.V0, model.kappa) == pytest.approx((want_m.r_drift, want_m.sigma, want_m.V0, want_m.kappa), nan_ok=True)
    assert len(extras) == len(fields)
    assert sol.spot_paths.shape == (12 // every + 1, 16) and sol.stopping_info[0].shape == (16,)


def test_the_euler_sources_take_a_bermudan_schedule_under_the_spot_state(fake):
    bs = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    em = hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), config(), 3)
    hh.solve(hh.PricingProblem(put(), bs), em, path_state="spot", exercise_every=4)
    (entry, args), = fake.lib.calls
    assert entry == "hh_lsm_solve_path" and _deref(args[1]).kind == _ffi.HH_SOURCE_EULER and args[4] == 4
    assert args[6] == float(hh.df(bs.rate, bs.referenceDate + (hh.yearfrac(REF, EXP) * 4 / 12) * hlsm.MILLISECONDS_IN_YEAR_365))
    fake.lib.calls.clear()
    hh.solve(hh.PricingProblem(put(), bs), em, path_state="spot")  # every step: the entry point it always took
    assert fake.lib.calls[0][0] == "hh_lsm_solve_euler"
    fake.lib.calls.clear()
    hh.simulate_spot_paths(hh.PricingProblem(put(), MARKETS["vg"]()), lsm_of("vg").mc_method, exercise_every=6)
    (entry, args), = fake.lib.calls
    assert entry == "hh_mc_path_grid" and _deref(args[1]).kind == _ffi.HH_SOURCE_VG and args[4] == 6


def test_refusals_come_before_any_device_work(fake):
    for name in PAIRS:
        prob = hh.PricingProblem(put(), MARKETS[name]())
        for every in (0, 5, 24, 1.5, -1):
            with pytest.raises(hh.MethodError, match="exercise_every"):
                hh.solve(prob, lsm_of(name), exercise_every=every)
            with pytest.raises(hh.MethodError, match="exercise_every"):
                hh.simulate_spot_paths(prob, lsm_of(name).mc_method, exercise_every=every)
        with pytest.raises(hh.MethodError, match='path_state="log"'):
            hh.solve(prob, lsm_of(name), path_state="log")
        route = routes.lsm_route_of(prob.market_inputs, lsm_of(name).mc_method)
        with pytest.raises(hh.MethodError, match=re.escape(route.one_device)):  # a second device: the route's words
            hh.solve(prob, lsm_of(name, devices=(0, 1)))
        with pytest.raises(hh.MethodError, match=re.escape(route.no_duals)):    # a Dual: the route's words
            hh.solve(hh.PricingProblem(put(), MARKETS[name](S=hh.Dual(100.0, (1.0,)))), lsm_of(name))
        with pytest.raises(hh.MethodError, match=re.escape(route.no_duals)):
            hh.solve(hh.PricingProblem(put(K=hh.Dual(100.0, (1.0,))), MARKETS[name]()), lsm_of(name))
        with pytest.raises(hh.MethodError, match="American VanillaOption"):
            hh.solve(hh.PricingProblem(put(hh.European()), MARKETS[name]()), lsm_of(name))
    bs = hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    em = hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), config(), 3)
    with pytest.raises(hh.MethodError, match='path_state="log"'):
        hh.solve(hh.PricingProblem(put(), bs), em, path_state="log", exercise_every=3)
    with pytest.raises(hh.MethodError, match="exercise_every"):
        hh.solve(hh.PricingProblem(put(), bs), em, path_state="spot", exercise_every=5)
    with pytest.raises(hh.MethodError):  # the Euler source is still opt-in
        hh.solve(hh.PricingProblem(put(), bs), em, exercise_every=3)
    with pytest.raises(hh.MethodError, match="exercise_every > 1"):  # the exact sources exercise on every date they draw
        hh.solve(hh.PricingProblem(put(), bs), hh.LSM(hh.LognormalDynamics(), hh.BlackScholesExact(), config(), 3), exercise_every=3)
    with pytest.raises(hh.MethodError):
        hh.simulate_spot_paths(hh.PricingProblem(put(), bs), hh.MonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(), config()))
    for kw in ({}, dict(exercise_every=3)):  # a second device on the Euler source: refused as solve refuses it, not run on one
        with pytest.raises(hh.MethodError, match="not sharded over several GPUs"):
            hh.simulate_spot_paths(hh.PricingProblem(put(), bs), hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), config(),
                                                                              devices=(0, 1)), **kw)
    with pytest.raises(hh.MethodError, match="not sharded over several GPUs"):
        hh.solve(hh.PricingProblem(put(), bs), hh.LSM(hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), config(), devices=(0, 1)), 3),
                 path_state="spot", exercise_every=3)
    assert fake.lib.calls == []


def test_what_was_refused_before_is_refused_in_the_same_words(fake):
    """an LSM whose dynamics are not the inputs' model's keeps its refusal; MonteCarlo on an American payoff keeps the
    route's no_american text; Merton's law at expiry is no path source"""
    cfg = config(8, 4)
    for mkt, method, text in (
            (MARKETS["bates"](), hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, 2), "LSM does not price the Bates model: use "),
            (MARKETS["vg"](), hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg, 2), "LSM does not price the Variance Gamma model: use "),
            (MARKETS["localvol"](), hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg, 2), "LSM does not price local volatility: use "),
            (MARKETS["bates"](), hh.LSM(hh.BatesDynamics(), hh.EulerMaruyama(), cfg, 2), "LSM does not price the Bates model: use "),
            (MARKETS["merton"](), hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(), cfg, 2), "full-path simulation on the HIP path"),
            (MARKETS["merton"](), hh.LSM(hh.MertonDynamics(), hh.MertonExact(), cfg, 2), "full-path simulation on the HIP path"),
            (MARKETS["qe"](), hh.LSM(hh.LognormalDynamics(), hh.HestonQE(1.5, True), cfg, 2), "full-path simulation on the HIP path")):
        for kw in ({}, dict(path_state="spot"), dict(exercise_every=2)):
            with pytest.raises(hh.MethodError, match=re.escape(text)):
                hh.solve(hh.PricingProblem(put(), mkt), method, **kw)
    for name in ("bates", "localvol", "vg", "qe"):
        dyn, strat, _, _ = PAIRS[name]
        route = routes.lsm_route_of(MARKETS[name](), lsm_of(name).mc_method)
        with pytest.raises(hh.MethodError, match=re.escape(route.no_american)):
            hh.solve(hh.PricingProblem(put(), MARKETS[name]()), hh.MonteCarlo(dyn(), strat(), cfg))
    assert routes.MERTON_LAW.source is None and routes.VG_LAW.source is None and routes.PLAIN.source is None
    assert [r.source for r in routes.SPOT_PATHS] == [_ffi.HH_SOURCE_LOCALVOL, _ffi.HH_SOURCE_BATES, _ffi.HH_SOURCE_QE, _ffi.HH_SOURCE_VG,
                                                     _ffi.HH_SOURCE_JUMP]
    assert routes.EULER.source == _ffi.HH_SOURCE_EULER
    assert fake.lib.calls == []
