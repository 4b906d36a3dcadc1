"""The Euler grid entry points on the host side, without a GPU: declared, exported and bound with the header's
arity; the host mirror packs them only behind a named path state."""
import ctypes as C
import os
import re

import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_euler_grid": 8, "hh_lsm_solve_euler": 10}


def test_new_prototypes_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None
    assert re.search(r"enum hh_path_state \{ HH_PATH_SPOT = 0, HH_PATH_LOG = 1 \};", hdr)
    assert (_ffi.HH_PATH_SPOT, _ffi.HH_PATH_LOG) == (0, 1)
    assert re.search(r"#define HH_ABI_VERSION 6\b", open(HEADER).read())


def _problem(mkt):
    put = hh.VanillaOption(100.0, hh.Date(2022, 1, 1), hh.American(), hh.Put(), hh.Spot())
    return hh.PricingProblem(put, mkt)


@pytest.mark.parametrize("split", [False, True])
def test_euler_sources_are_packed_only_when_asked_for(split):
    from hedgehog_jl_amd.lsm import _lsm_structs
    ref = hh.Date(2021, 1, 1)
    cfg = hh.SimulationConfig(100, steps=10, variance_reduction=hh.Antithetic())
    heston = _problem(hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7))
    bs = _problem(hh.BlackScholesInputs(ref, 0.03, 100.0, 0.2))
    for prob, dyn, code in ((heston, hh.HestonDynamics(), _ffi.HH_HESTON), (bs, hh.LognormalDynamics(), _ffi.HH_LOGNORMAL)):
        mc = hh.MonteCarlo(dyn, hh.EulerMaruyama(), cfg, em_split=split)
        with pytest.raises(hh.MethodError):
            _lsm_structs(prob, mc)
        model, c, T = _lsm_structs(prob, mc, euler=True)
        assert (c.dynamics, c.strategy, c.em_split, c.antithetic) == (code, _ffi.HH_EULER_MARUYAMA, int(split), 1)
        assert (c.n_paths, c.n_steps, c.seeds_len) == (100, 10, 100) and T == 1.0
        assert model.S0 == 100.0 and model.r_drift == pytest.approx(0.03)
    # a Dual input is refused on the Euler source as on every full-path source
    dual = _problem(hh.HestonInputs(ref, 0.03, hh.Dual(100.0, (1.0,)), 0.04, 2.0, 0.04, 0.3, -0.7))
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        _lsm_structs(dual, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg), euler=True)


def test_path_state_is_checked_before_any_device_work():
    ref = hh.Date(2021, 1, 1)
    prob = _problem(hh.HestonInputs(ref, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7))
    cfg = hh.SimulationConfig(100, steps=10)
    euler = hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, 3)
    exact = hh.LSM(hh.HestonDynamics(), hh.HestonBroadieKaya(), cfg, 3)
    with pytest.raises(ValueError):
        hh.solve(prob, euler, path_state="exp")
    with pytest.raises(hh.MethodError):
        hh.solve(prob, exact, path_state="log")
    with pytest.raises(hh.MethodError):
        hh.solve(prob, euler)
    with pytest.raises(hh.MethodError):
        hh.simulate_euler_paths(prob, exact.mc_method)
    with pytest.raises(hh.MethodError):
        hh.solve(prob, hh.LSM(hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, devices=range(2)), 3),
                 path_state="spot")
