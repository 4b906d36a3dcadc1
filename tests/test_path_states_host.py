"""American exercise under stochastic volatility on the host side, without a GPU: the two entry points and the descriptor
kind declared, exported and bound; the host routing of regressors="spot_variance", every MethodError, and
simulate_state_paths' shapes against a fake library."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import path_grid_cases as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_states": 8, "hh_lsm_solve_path_states": 12}
REF, EXP = hh.Date(2025, 1, 1), hh.Date(2026, 1, 1)


def test_new_prototypes_are_declared_exported_and_bound():
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines()}
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto and len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None and name in exported
    assert re.search(r"HH_LSM_STATES_LOG_ASSETS = 0, HH_LSM_STATES_LOG_SPOT_VARIANCE = 1 \}", hdr)
    assert (_ffi.HH_LSM_STATES_LOG_ASSETS, _ffi.HH_LSM_STATES_LOG_SPOT_VARIANCE) == (0, 1)
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    assert lib.hh_assets_rows_elems(513, 12, 2, 1) == 13 * 2 * 1026
    # the header states the layout, the raw-variance convention and the errors; "variance rows" has left the neighbours' lists
    block = text[text.index("American exercise under stochastic volatility: the state rows"):]
    for words in ("rows[(date·2 + state)·n_total + column]", "RAW STATE", "unclipped", "walk has no variance", "HH_ERR_UNSUPPORTED"):
        assert words in block, words
    for m in re.finditer(r"Not provided:(.*?)(?:Provided elsewhere:|\*/)", text, re.S):
        if "variance rows" in m.group(1):
            assert "exact Heston and Broadie–Kaya" in m.group(1)
    assert "Provided elsewhere: variance rows for QE and Bates, and for Heston Euler — hh_mc_path_states" in text


# ---- the host's routes against a fake library ----------------------------------------------------------------------------------

class FakeLib:
    def __init__(self):
        self.calls = []

    def _record(self, entry, source, model, cfg, every, **kw):
        s, m, c = source._obj, model._obj, cfg._obj
        self.calls.append(dict(entry=entry, source=s.kind, qe=bool(s.qe), jump=bool(s.jump), every=every, strike=m.strike, cp=m.cp,
                               T=m.T, V0=m.V0, dynamics=c.dynamics, strategy=c.strategy, n=c.n_paths, steps=c.n_steps,
                               anti=c.antithetic, **kw))
        return c.n_steps // every + 1, c.n_paths * (2 if c.antithetic else 1)

    def hh_lsm_solve_path_states(self, handle, source, model, cfg, every, degree, discount, res, tau, val, coef, rows):
        dates, n = self._record("hh_lsm_solve_path_states", source, model, cfg, every, degree=degree, discount=discount,
                                outs=(tau, val, coef, rows))
        if rows:
            out = np.ctypeslib.as_array(C.cast(rows, C.POINTER(C.c_double)), shape=(dates * 2 * n,)).reshape(dates, 2, n)
            out[:, 0], out[:, 1] = math.log(2.0), 0.25
        res._obj.price, res._obj.std_error = 13.7, 0.04
        return 0

    def hh_lsm_solve_path(self, handle, source, model, cfg, every, degree, discount, res, tau, val, grid):
        self._record("hh_lsm_solve_path", source, model, cfg, every, degree=degree)
        res._obj.price, res._obj.std_error = 11.9, 0.04
        return 0

    def hh_lsm_solve_euler(self, handle, model, cfg, state, degree, discount, res, tau, val, grid):
        self.calls.append(dict(entry="hh_lsm_solve_euler", state=state, degree=degree))
        res._obj.price, res._obj.std_error = 11.9, 0.04
        return 0

    def hh_mc_path_states(self, handle, source, model, cfg, every, rows, on_device, res):
        dates, n = self._record("hh_mc_path_states", source, model, cfg, every, on_device=on_device)
        out = np.ctypeslib.as_array(C.cast(rows, C.POINTER(C.c_double)), shape=(dates * 2 * n,)).reshape(dates, 2, n)
        out[:, 0], out[:, 1] = math.log(2.0), -0.125
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


def _cfg(n=16, steps=12, vr=None):
    return hh.SimulationConfig(n, steps=steps, seeds=np.arange(n), variance_reduction=vr)


def _put(K=100.0, style=None):
    return hh.VanillaOption(K, EXP, style or hh.American(), hh.Put(), hh.Spot())


HESTON = hh.HestonInputs(REF, 0.05, 100.0, 0.16, 0.5, 0.16, 1.5, 0.0)
BATES = hh.BatesInputs(REF, 0.05, 100.0, 0.16, 0.5, 0.16, 1.5, 0.0, 0.8, -0.1, 0.2)


def _lsm(dyn, strat, degree=3, cfg=None, **kw):
    return hh.LSM(hh.MonteCarlo(dyn, strat, cfg or _cfg(), **kw), degree)


EULER = lambda **kw: _lsm(hh.HestonDynamics(), hh.EulerMaruyama(), **kw)  # noqa: E731
QE = lambda **kw: _lsm(hh.HestonDynamics(), hh.HestonQE(), **kw)  # noqa: E731
BATES_QE = lambda **kw: _lsm(hh.BatesDynamics(), hh.HestonQE(), **kw)  # noqa: E731


def test_the_solve_routes(fake):
    prob = hh.PricingProblem(_put(), HESTON)
    sol = hh.solve(prob, EULER(), exercise_every=3, regressors="spot_variance", path_state="spot")
    assert isinstance(sol, hh.LSMSolution) and (sol.price, sol.std_error) == (13.7, 0.04)
    (call,) = fake.calls
    assert (call["entry"], call["source"], call["every"], call["degree"]) == ("hh_lsm_solve_path_states", _ffi.HH_SOURCE_EULER, 3, 3)
    assert (call["dynamics"], call["strategy"]) == (_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA)
    assert (call["strike"], call["cp"], call["V0"], call["n"], call["steps"], call["anti"]) == (100.0, -1.0, 0.16, 16, 12, 0)
    assert call["discount"] == pytest.approx(math.exp(-0.05 * call["T"] * 3 / 12), rel=1e-12)
    tau, val, coef, rows = call["outs"]
    assert tau is not None and val is not None and coef is None and rows is None
    assert sol.stopping_info[0].shape == (16,) and sol.spot_paths is None
    fake.calls.clear()
    # HestonQE and Bates: the route's own source and structs; spot_paths is exp of the stored log spot, (dates + 1, columns)
    for mkt, method, kind, jump in ((HESTON, QE(cfg=_cfg(vr=hh.Antithetic())), _ffi.HH_SOURCE_QE, False),
                                    (BATES, BATES_QE(cfg=_cfg(vr=hh.Antithetic())), _ffi.HH_SOURCE_BATES, True)):
        sol = hh.solve(hh.PricingProblem(_put(95.0), mkt), method, regressors="spot_variance", spot_paths=True, stopping_info=False)
        (call,) = fake.calls
        assert (call["entry"], call["source"], call["qe"], call["jump"]) == ("hh_lsm_solve_path_states", kind, True, jump)
        assert (call["strategy"], call["every"], call["anti"], call["strike"]) == (_ffi.HH_QE, 1, 1, 95.0)
        assert sol.stopping_info is None and sol.spot_paths.shape == (13, 32) and np.all(sol.spot_paths == np.exp(math.log(2.0)))
        fake.calls.clear()
    # the default takes exactly the paths it took: the spot rows of the route, hh_lsm_solve_euler under a named path state
    hh.solve(prob, QE(), exercise_every=3)
    hh.solve(prob, QE(), exercise_every=3, regressors="spot")
    hh.solve(prob, EULER(), path_state="spot")
    assert [c["entry"] for c in fake.calls] == ["hh_lsm_solve_path", "hh_lsm_solve_path", "hh_lsm_solve_euler"]
    fake.calls.clear()
    # degree 8 is the last one: C(2 + 8, 8) = 45 basis functions
    hh.solve(prob, QE(degree=8), regressors="spot_variance")
    assert fake.calls[0]["degree"] == 8


def test_simulate_state_paths(fake):
    prob = hh.PricingProblem(_put(style=hh.European()), HESTON)
    for method, kind in ((EULER(cfg=_cfg(8, vr=hh.Antithetic())), _ffi.HH_SOURCE_EULER), (QE(cfg=_cfg(8, vr=hh.Antithetic())), _ffi.HH_SOURCE_QE)):
        paths = hh.simulate_state_paths(prob, method.mc_method, exercise_every=4)
        assert isinstance(paths, hh.StatePaths) and paths.spot.shape == paths.variance.shape == (4, 16)
        assert np.all(paths.spot == np.exp(math.log(2.0))) and np.all(paths.variance == -0.125)  # the variance as the walk holds it
        assert np.allclose(paths.times, np.linspace(0.0, paths.times[-1], 4)) and paths.times[-1] == pytest.approx(1.0, abs=0.01)
        (call,) = fake.calls
        assert (call["entry"], call["source"], call["every"], call["on_device"]) == ("hh_mc_path_states", kind, 4, 0)
        fake.calls.clear()
    assert "unclipped" in hh.StatePaths.__doc__


def test_refusals_touch_no_device(fake):
    prob = hh.PricingProblem(_put(), HESTON)
    sv = dict(regressors="spot_variance")
    bs = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    merton = hh.MertonInputs(REF, 0.05, 100.0, 0.2, 0.8, -0.1, 0.2)
    vg = hh.VarianceGammaInputs(REF, 0.05, 100.0, 0.2, -0.3, 0.5)
    surf = pg.table(4, 16)
    localvol = hh.LocalVolInputs(REF, 0.05, 100.0, hh.LocalVolSurface(surf["times"], surf["x_lo"] + surf["h"] * np.arange(16), surf["vols"]))
    several = hh.MultiAssetInputs(REF, 0.05, [100.0, 100.0], [0.2, 0.3], [[1.0, 0.3], [0.3, 1.0]])
    index_put = hh.IndexOption(hh.WorstOf(), _put())
    dual = hh.Dual(100.0, (1.0,))
    cases = [
        (hh.PricingProblem(_put(), bs), _lsm(hh.LognormalDynamics(), hh.EulerMaruyama()), dict(sv, path_state="spot"), "has no variance"),
        (hh.PricingProblem(_put(), bs), _lsm(hh.LognormalDynamics(), hh.BlackScholesExact()), sv, "has no variance"),
        (hh.PricingProblem(_put(), merton), _lsm(hh.MertonDynamics(), hh.EulerMaruyama()), sv, "has no variance"),
        (hh.PricingProblem(_put(), vg), _lsm(hh.VarianceGammaDynamics(), hh.VarianceGammaExact()), sv, "has no variance"),
        (hh.PricingProblem(_put(), localvol), _lsm(hh.LocalVolDynamics(), hh.EulerMaruyama()), sv, "has no variance"),
        (hh.PricingProblem(index_put, several), _lsm(hh.MultiAssetDynamics(), hh.EulerMaruyama()), sv, "has no variance"),
        (prob, _lsm(hh.HestonDynamics(), hh.HestonBroadieKaya()), sv, "has no variance rows"),
        (prob, EULER(), dict(sv, path_state="log"), 'path_state="log" is not offered'),
        (prob, QE(), dict(sv, path_state="log"), 'path_state="log" is not offered'),
        (prob, EULER(), sv, 'goes with path_state="spot"'),
        (prob, EULER(devices=range(2)), dict(sv, path_state="spot"), "not sharded"),
        (prob, QE(devices=range(2)), sv, "one device"),
        (hh.PricingProblem(_put(), hh.HestonInputs(REF, 0.05, dual, 0.16, 0.5, 0.16, 1.5, 0.0)), EULER(), dict(sv, path_state="spot"),
         "FiniteDifference"),
        (hh.PricingProblem(_put(), hh.HestonInputs(REF, 0.05, dual, 0.16, 0.5, 0.16, 1.5, 0.0)), QE(), sv, "FiniteDifference"),
        (hh.PricingProblem(_put(dual), HESTON), QE(), sv, "FiniteDifference"),
        (prob, QE(degree=9), sv, "1 <= degree <= 8"),
        (prob, QE(degree=0), sv, "1 <= degree <= 8"),
        (prob, QE(), dict(sv, exercise_every=5), "must be a whole number >= 1 that divides steps"),
        (prob, EULER(), dict(sv, path_state="spot", exercise_every=0), "must be a whole number >= 1 that divides steps"),
        (hh.PricingProblem(_put(style=hh.European()), HESTON), QE(), sv, "needs an American VanillaOption"),
    ]
    for k, (p, method, kw, words) in enumerate(cases):
        with pytest.raises(hh.MethodError, match=re.escape(words)):
            hh.solve(p, method, **kw)
    with pytest.raises(ValueError, match="regressors must be"):
        hh.solve(prob, QE(), regressors="variance")
    with pytest.raises(ValueError, match="regressors must be"):
        hh.solve(prob, QE(), regressors=None)
    with pytest.raises(hh.MethodError, match="has no variance"):
        hh.simulate_state_paths(hh.PricingProblem(_put(), bs), _lsm(hh.LognormalDynamics(), hh.EulerMaruyama()).mc_method)
    with pytest.raises(hh.MethodError, match="divides steps"):
        hh.simulate_state_paths(prob, QE().mc_method, exercise_every=7)
    assert fake.calls == []
