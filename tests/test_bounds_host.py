"""Dual bounds for American exercise on the host side, without a GPU: the entry points declared, exported and bound with the
header's arity; hh_lsm_policy_elems; the host's routes, every MethodError and the seed-coincidence refusal against a fake
library; the numpy restatements of tests/bounds_cases.py against cases computed by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import bounds_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_lsm_fit_states": 11, "hh_lsm_fit_path_states": 9, "hh_lsm_policy_value": 11, "hh_lsm_policy_value_path": 9,
       "hh_lsm_upper_bound": 13}
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
    proto = re.search(r"\bsize_t\s+hh_lsm_policy_elems\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert proto and len(proto.group(1).split(",")) == 3
    assert bound["hh_lsm_policy_elems"][1] is C.c_size_t and "hh_lsm_policy_elems" in exported
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    assert C.sizeof(_ffi.hh_bounds_result) == 56 and "/* 56 bytes */" in text
    block = text[text.index("Dual bounds for American exercise: the fitted policy as an array"):]
    for words in ("policy[t·(2m + B) + 2m + j]", "INNER KEYS", "0x9E3779B97F4A7C15", "(s + 2^31, 0, 0, domain 0)", "Jensen",
                  "n_inner = 0 or not a multiple of 64", "antithetic outer paths"):
        assert words in block, words


def test_policy_elems():
    lib = _ffi.load_library()
    for n_dates, m, degree in ((1, 1, 1), (6, 2, 2), (12, 2, 3), (12, 2, 8), (5, 3, 4), (7, 8, 2), (65534, 2, 8)):
        want = (n_dates + 1) * (2 * m + math.comb(m + degree, degree))
        assert lib.hh_lsm_policy_elems(n_dates, m, degree) == want
        if m == 2:
            assert bc.blank_policy(n_dates if n_dates < 100 else 3, degree).shape[1] == want // (n_dates + 1)
    # no such basis: degree outside 1 .. 8, m outside 1 .. HH_MAX_ASSETS, more than HH_LSM_MAX_BASIS functions
    for n_dates, m, degree in ((6, 2, 0), (6, 2, 9), (6, 0, 2), (6, 9, 2), (6, 3, 5), (6, 8, 3)):
        assert lib.hh_lsm_policy_elems(n_dates, m, degree) == 0


# ---- the numpy restatements against cases computed by hand --------------------------------------------------------------------

def _rows(spots, v=0.04):
    spots = np.asarray(spots, dtype=np.float64)  # [date][column]
    return np.stack([np.log(spots), np.full(spots.shape, v)], axis=1)


def test_forward_value_by_hand():
    """a put at K = 100, three dates, degree 1 (basis 1, z_0, z_1), μ = 0 and isd = 1: z_0 = S.
    Column 0: S = 95, 90, 80.  Date 1: fit = 0.04·95 = 3.8 < pay = 5: stops at date 1 with 5.
    Column 1: S = 105, 98, 110.  Date 1: out of the money.  Date 2: fit = 10 > pay = 2: goes on.  Expiry: max(−10, 0) = 0."""
    rows = _rows([[100.0, 100.0], [95.0, 105.0], [90.0, 98.0], [80.0, 110.0]])
    policy = bc.blank_policy(3, 1)
    assert policy.shape == (4, 7)
    policy[1, 4:] = (0.0, 0.04, 0.0)
    policy[2, 4:] = (10.0, 0.0, 0.0)
    tau, val = bc.forward_value(rows, policy, -1.0, 100.0, 1)
    assert tau.tolist() == [1, 3] and val == pytest.approx([5.0, 0.0], abs=1e-12)
    # standardising: μ_0 = 90, isd_0 = 0.1 at date 2 and the coefficient on z_0 — column 1: z_0 = 0.8, fit = 1.6 < pay = 2
    policy[2, :7] = (90.0, 0.0, 0.1, 1.0, 0.0, 2.0, 0.0)
    tau, val = bc.forward_value(rows, policy, -1.0, 100.0, 1)
    assert tau.tolist() == [1, 2] and val == pytest.approx([5.0, 2.0], abs=1e-12)
    # the hand-made policies: never, and the first date in the money
    tau, val = bc.forward_value(rows, bc.never_policy(3, 1), -1.0, 100.0, 1)
    assert tau.tolist() == [3, 3] and val == pytest.approx([20.0, 0.0], abs=1e-12)
    for p in (bc.zero_policy(3, 1), bc.blank_policy(3, 1)):
        tau, val = bc.forward_value(rows, p, -1.0, 100.0, 1)
        assert tau.tolist() == [1, 2] and val == pytest.approx([5.0, 2.0], abs=1e-12)
    # a call on the same rows under the zero policy: column 1 at date 1
    tau, val = bc.forward_value(rows, bc.zero_policy(3, 1), 1.0, 100.0, 1)
    assert tau.tolist() == [3, 1] and val == pytest.approx([0.0, 5.0], abs=1e-12)


def test_dual_outer_by_hand():
    """one column, two dates, D = 1/2, a put at 100 on S = 100, 90, 120 with Ĉ = 8, 6.
    Never exercise: L_1 = Ĉ_1 = 6, M_1 = 0.5·6 − 8 = −5, gap_1 = 0.5·10 + 5 = 10; L_2 = 0, M_2 = −5 − 0.5·6 = −8, gap_2 = 8: 10.
    Exercise at date 1: L_1 = 10, M_1 = 5 − 8 = −3, gap_1 = 8; M_2 = −3 − 3 = −6, gap_2 = 6: 8."""
    rows = _rows([[100.0], [90.0], [120.0]])
    cont = np.array([[8.0], [6.0]])
    assert bc.dual_outer(rows, cont, bc.never_policy(2, 1), -1.0, 100.0, 1, 0.5) == pytest.approx([10.0], abs=1e-12)
    assert bc.dual_outer(rows, cont, bc.zero_policy(2, 1), -1.0, 100.0, 1, 0.5) == pytest.approx([8.0], abs=1e-12)
    # the start counts: deep in the money at date 0, nothing later — max_t includes t = 0
    rows = _rows([[60.0], [100.0], [100.0]])
    assert bc.dual_outer(rows, np.array([[40.0], [0.0]]), bc.never_policy(2, 1), -1.0, 100.0, 1, 0.5) == pytest.approx([40.0], abs=1e-12)


def test_closed_forms():
    # put-call parity and the tree against Black–Scholes with no early date
    S, K, r, vol, T = 100.0, 100.0, 0.05, 0.2, 1.0
    put = float(bc.bs_put(S, K, r, vol, T))
    assert put == pytest.approx(5.573526, abs=1e-6)
    mean, var, p = bc.put_moments(np.array([S]), K, r, vol, T)
    assert mean[0] == pytest.approx(put, rel=1e-12) and 0.4 < p[0] < 0.5
    rng = np.random.default_rng(1)
    y = math.exp(-r * T) * np.maximum(K - S * np.exp((r - 0.5 * vol * vol) * T + vol * math.sqrt(T) * rng.standard_normal(400_000)), 0.0)
    assert var[0] == pytest.approx(y.var(), rel=0.02)
    assert bc.bermudan_tree(S, K, r, vol, T, 1200, 1200) == pytest.approx(put, abs=2e-3)
    berm = bc.bermudan_tree(S, K, r, vol, T, 1200, 100)
    assert put < berm < 6.1 and abs(berm - bc.bermudan_tree(S, K, r, vol, T, 2400, 200)) < 5e-4


# ---- the host's routes against a fake library ----------------------------------------------------------------------------------

class FakeLib:
    def __init__(self):
        self.calls = []

    def _seeds(self, c):
        return np.ctypeslib.as_array(C.cast(c.seeds, C.POINTER(C.c_uint64)), shape=(int(c.n_paths),)).copy()

    def hh_lsm_fit_path_states(self, handle, source, model, cfg, every, degree, D, res, policy):
        s, m, c = source._obj, model._obj, cfg._obj
        n_dates = c.n_steps // every
        shape = bc.policy_shape(n_dates, degree)
        out = np.ctypeslib.as_array(C.cast(policy, C.POINTER(C.c_double)), shape=(shape[0] * shape[1],)).reshape(shape)
        out[:] = bc.blank_policy(n_dates, degree)
        out[1:n_dates, 4] = 7.0
        self.calls.append(dict(entry="hh_lsm_fit_path_states", source=s.kind, every=every, degree=degree, D=D, seeds=self._seeds(c),
                               strike=m.strike, cp=m.cp, anti=c.antithetic))
        res._obj.price, res._obj.std_error = 12.66, 0.03
        return 0

    def hh_lsm_policy_value_path(self, handle, source, model, cfg, every, policy, degree, D, res):
        s, c = source._obj, cfg._obj
        self.calls.append(dict(entry="hh_lsm_policy_value_path", source=s.kind, every=every, degree=degree, D=D, seeds=self._seeds(c)))
        res._obj.price, res._obj.std_error = 12.5, 0.04
        return 0

    def hh_lsm_upper_bound(self, handle, model, cfg, every, policy, degree, D, n_inner, inner_seed, res, cont, cont_se, pmax):
        c = cfg._obj
        self.calls.append(dict(entry="hh_lsm_upper_bound", every=every, degree=degree, D=D, n_inner=n_inner, inner_seed=inner_seed,
                               seeds=self._seeds(c), dynamics=c.dynamics, strategy=c.strategy, outs=(cont, cont_se, pmax)))
        res._obj.upper, res._obj.upper_se = 12.9, 0.05
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


def _cfg(n=16, steps=12, vr=None, first=1):
    return hh.SimulationConfig(n, steps=steps, seeds=np.arange(first, first + n), variance_reduction=vr)


def _put(K=100.0, style=None):
    return hh.VanillaOption(K, EXP, style or hh.American(), hh.Put(), hh.Spot())


HESTON = hh.HestonInputs(REF, 0.05, 100.0, 0.16, 0.5, 0.16, 1.5, 0.0)
BATES = hh.BatesInputs(REF, 0.05, 100.0, 0.16, 0.5, 0.16, 1.5, 0.0, 0.8, -0.1, 0.2)


def _lsm(dyn, strat, degree=3, cfg=None, **kw):
    return hh.LSM(hh.MonteCarlo(dyn, strat, cfg or _cfg(), **kw), degree)


EULER = lambda **kw: _lsm(hh.HestonDynamics(), hh.EulerMaruyama(), **kw)  # noqa: E731
QE = lambda **kw: _lsm(hh.HestonDynamics(), hh.HestonQE(), **kw)  # noqa: E731


def test_the_bounds_route(fake):
    prob = hh.PricingProblem(_put(), HESTON)
    sol = hh.solve(prob, hh.DualBounds(EULER(), outer=8, inner=128, fresh=np.arange(100, 120), inner_seed=5), exercise_every=3)
    assert isinstance(sol, hh.BoundsSolution)
    assert (sol.lower, sol.lower_se, sol.upper, sol.upper_se, sol.in_sample, sol.in_sample_se) == (12.5, 0.04, 12.9, 0.05, 12.66, 0.03)
    assert sol.gap == pytest.approx(0.4) and sol.gap_se == pytest.approx(math.hypot(0.04, 0.05))
    fit, low, up = fake.calls
    assert [c["entry"] for c in fake.calls] == ["hh_lsm_fit_path_states", "hh_lsm_policy_value_path", "hh_lsm_upper_bound"]
    assert fit["seeds"].tolist() == list(range(1, 17)) and low["seeds"].tolist() == list(range(100, 120))
    assert up["seeds"].tolist() == list(range(120, 128))  # a count: the seeds after the largest one used so far
    assert (fit["source"], low["source"]) == (_ffi.HH_SOURCE_EULER, _ffi.HH_SOURCE_EULER)
    assert (up["dynamics"], up["strategy"], up["n_inner"], up["inner_seed"]) == (_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, 128, 5)
    assert {c["every"] for c in fake.calls} == {3} and {c["degree"] for c in fake.calls} == {3}
    assert len({c["D"] for c in fake.calls}) == 1 and fit["D"] == pytest.approx(math.exp(-0.05 * 3 / 12), rel=1e-3)
    assert up["outs"] == (None, None, None)
    policy = sol.policy
    assert isinstance(policy, hh.ExercisePolicy) and (policy.m, policy.degree, policy.dates, policy.exercise_every) == (2, 3, 4, 3)
    assert policy.array.shape == (5, 14) and np.all(policy.array[1:4, 4] == 7.0) and policy.discount == fit["D"]
    fake.calls.clear()
    # the pieces on their own; a hand-made policy has no fit seeds and is valued on any
    pol = hh.fit_policy(prob, EULER(), exercise_every=3)
    assert pol.in_sample.price == 12.66 and pol.fit_seeds.tolist() == list(range(1, 17))
    low = hh.policy_value(prob, EULER(), pol, seeds=np.arange(50, 60))
    assert (low.price, low.std_error) == (12.5, 0.04) and fake.calls[-1]["seeds"].tolist() == list(range(50, 60))
    hand = hh.ExercisePolicy(bc.never_policy(4, 3), 2, 3, 4, pol.discount, 3)
    hh.policy_value(prob, EULER(), hand)
    assert fake.calls[-1]["seeds"].tolist() == list(range(1, 17))
    res, cont, cont_se, pmax = hh.upper_bound(prob, EULER(), hand, np.arange(200, 264), inner=64, want_cont=True)
    assert cont.shape == cont_se.shape == (4, 64) and pmax.shape == (64,) and res.upper == 12.9
    # fit_policy and policy_value serve HestonQE too (state rows); the upper bound does not
    polq = hh.fit_policy(prob, QE(), exercise_every=3)
    hh.policy_value(prob, QE(), polq, seeds=np.arange(50, 60))
    assert fake.calls[-1]["source"] == _ffi.HH_SOURCE_QE


def test_refusals_touch_no_device(fake):
    prob = hh.PricingProblem(_put(), HESTON)
    bs = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    several = hh.MultiAssetInputs(REF, 0.05, [100.0, 100.0], [0.2, 0.3], [[1.0, 0.3], [0.3, 1.0]])
    db = lambda lsm, **kw: hh.DualBounds(lsm, **dict(dict(outer=8, inner=64, fresh=np.arange(100, 116)), **kw))  # noqa: E731
    cases = [
        # seeds that coincide with the fit's
        (prob, db(EULER(), fresh=np.arange(10, 26)), {}, "coincide with the seeds the policy was fitted on"),
        (prob, db(EULER(), outer=np.arange(16, 24)), {}, "coincide with the seeds the policy was fitted on"),
        # routes that cannot serve say what is missing
        (prob, db(QE()), {}, "no nested walk"),
        (hh.PricingProblem(_put(), BATES), db(_lsm(hh.BatesDynamics(), hh.HestonQE())), {}, "no nested walk"),
        (hh.PricingProblem(_put(), bs), db(_lsm(hh.LognormalDynamics(), hh.EulerMaruyama())), {}, "no variance rows"),
        (hh.PricingProblem(_put(), bs), db(_lsm(hh.LognormalDynamics(), hh.BlackScholesExact())), {}, "no variance rows"),
        (prob, db(_lsm(hh.HestonDynamics(), hh.HestonBroadieKaya())), {}, "no variance rows"),
        (hh.PricingProblem(hh.IndexOption(hh.WorstOf(), _put()), several), db(_lsm(hh.MultiAssetDynamics(), hh.EulerMaruyama())), {},
         "several-asset walk"),
        (prob, db(EULER(cfg=_cfg(vr=hh.Antithetic()))), {}, "antithetic outer paths"),
        (prob, db(EULER(), inner=100), {}, "multiple of 64"),
        (prob, db(EULER(), inner=0), {}, "multiple of 64"),
        (prob, db(EULER(degree=9)), {}, "1 <= degree <= 8"),
        (prob, db(EULER()), dict(exercise_every=5), "must be a whole number >= 1 that divides steps"),
        (hh.PricingProblem(_put(style=hh.European()), HESTON), db(EULER()), {}, "needs an American VanillaOption"),
        (prob, db(EULER(devices=range(2))), {}, "not sharded"),
        (prob, hh.DualBounds("LSM"), {}, "DualBounds(LSM(...)"),
    ]
    for p, method, kw, words in cases:
        with pytest.raises(hh.MethodError, match=re.escape(words)):
            hh.solve(p, method, **kw)
    assert fake.calls == []
    pol = hh.fit_policy(prob, EULER(), exercise_every=3)
    fake.calls.clear()
    with pytest.raises(hh.MethodError, match="coincide with the seeds the policy was fitted on"):
        hh.policy_value(prob, EULER(), pol)                       # the fit's own seeds
    with pytest.raises(hh.MethodError, match="coincide with the seeds the policy was fitted on"):
        hh.policy_value(prob, EULER(), pol, seeds=np.arange(16, 40))  # one shared seed is enough
    with pytest.raises(hh.MethodError, match="the policy has 4 dates at degree 3"):
        hh.policy_value(prob, EULER(), pol, seeds=np.arange(50, 60), exercise_every=4)
    with pytest.raises(hh.MethodError, match="the policy has 4 dates at degree 3"):
        hh.policy_value(prob, EULER(degree=2), pol, seeds=np.arange(50, 60))
    with pytest.raises(hh.MethodError, match='regressors="spot_variance"'):
        hh.fit_policy(prob, EULER(), regressors="spot")
    with pytest.raises(hh.MethodError, match="no nested walk"):
        hh.upper_bound(prob, QE(), pol, np.arange(50, 60))
    with pytest.raises(ValueError, match="finite"):
        hh.ExercisePolicy(np.full((5, 14), np.nan), 2, 3, 4, 0.99)
    with pytest.raises(ValueError, match=r"\(5, 14\) array"):
        hh.ExercisePolicy(np.zeros((5, 13)), 2, 3, 4, 0.99)
    assert fake.calls == []
