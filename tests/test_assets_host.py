"""Several correlated lognormal assets on the host side, without a GPU: the two entry points declared, exported and
bound; what a call forms on the host (csrc/hh_assets.h) as a stand-alone program (also under AddressSanitizer and UBSan)
against the Python-float restatement, bit for bit; the golden closed forms, their maker and MultiAssetAnalytic; the
restatement's own sanity; every Python route against a fake library."""
import ctypes as C
import json
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
from tests import assets_cases as ac  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_assets": 9, "hh_mc_solve_path_assets": 11}
REF, EXP = hh.Date(2025, 1, 1), hh.Date(2026, 1, 1)
DOC = ac.load_golden()


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
    assert re.search(r"#define HH_MAX_ASSETS 8\b", hdr) and _ffi.HH_MAX_ASSETS == 8
    assert (_ffi.HH_INDEX_WEIGHTED_SUM, _ffi.HH_INDEX_GEOMETRIC, _ffi.HH_INDEX_BEST_OF, _ffi.HH_INDEX_WORST_OF) == (0, 1, 2, 3)
    assert C.sizeof(_ffi.hh_assets) == 8 + 3 * 64 + 512
    assert _ffi.hh_assets.corr.offset == 8 + 3 * 64 and _ffi.hh_assets.spots.offset == 8
    assert '"hh_assets.hip"' in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "#include <hip" not in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_assets.h")).read()
    assert re.search(r"kDomAssets = 6u;", open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_rng.h")).read())


# ---- the host's part as a program ------------------------------------------------------------------------------------------

NEARLY_SINGULAR = [[1.0, 1.0 - 2.0 ** -40], [1.0 - 2.0 ** -40, 1.0]]
VALID = [  # (case, kind, n_steps)
    (dict(ac.path_case(1)), ac.SUM, 1),
    (dict(ac.CASE_B), ac.BEST, 4),
    (dict(ac.CASE_B, corr=NEARLY_SINGULAR), ac.SUM, 7),
    (dict(ac.CASE_A), ac.GEO, 6),
    (dict(ac.CASE_A, weights=[2.0, 0.5, 3.0]), ac.WORST, 252),
    (dict(ac.CASE_E), ac.GEO, 5),
    (dict(ac.path_case(8), r_drift=-0.01, T=0.3), ac.BEST, 3),
]
NAN = float("nan")
INVALID = [  # (correlation matrix, the reason the program gives)
    ([[1.0, 0.5], [0.25, 1.0]], "not symmetric"),
    ([[1.0, 0.5], [0.5, 0.999]], "diagonal"),
    ([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]], "not positive definite"),  # indefinite
    ([[1.0, 1.0], [1.0, 1.0]], "not positive definite"),                               # singular
    ([[1.0, 0.5, 0.5], [0.5, 1.0, -0.5], [0.5, -0.5, 1.0]], "not positive definite"),  # singular, rank 2
    ([[1.0, NAN], [NAN, 1.0]], "not finite"),
    ([[1.0, 1.5], [1.5, 1.0]], "outside"),
]


def _record(case, kind, n_steps):
    d = len(case["spots"])
    nums = list(case["spots"]) + list(case["sigmas"]) + list(case["weights"]) + [t for row in case["corr"] for t in row]
    return f"{d} {kind} {n_steps} {float(case['r_drift']).hex()} {float(case['T']).hex()} " + " ".join(float(t).hex() for t in nums)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_host_program(tmp_path, build):
    """tests/c/assets_host_check.cpp — its own main, csrc/hh_assets.h included — factors every matrix and forms every
    constant: L, drift, A and x0 are the Python-float restatement's bit for bit, d = 1, 2, 3 and 8, a nearly singular
    matrix among them; every invalid matrix is reported with its reason.  Built plainly and with
    -fsanitize=address,undefined, and run as a program: nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = tmp_path / ("assets_host_check_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "assets_host_check.cpp"), "-o", str(exe)], check=True)
    bad_cases = [(dict(ac.path_case(len(Cm)), corr=Cm), ac.SUM, 2) for Cm, _ in INVALID]
    with open(tmp_path / "records.txt", "w") as f:
        for rec in VALID + bad_cases:
            f.write(_record(*rec) + "\n")
    run = subprocess.run([str(exe), str(tmp_path / "records.txt")], capture_output=True, text=True, env=host_env(), timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(VALID) + len(INVALID)
    assert {len(c["spots"]) for c, _, _ in VALID} == {1, 2, 3, 8}
    for (case, kind, n_steps), line in zip(VALID, lines):
        d = len(case["spots"])
        L = ac.cholesky_fp64(case["corr"])
        assert L is not None and ac.corr_defect(case["corr"]) is None
        drift, A, x0 = ac.constants_fp64(case, kind, n_steps, L)
        tok = line.split()
        assert tok[0] == "ok", line
        got = [float.fromhex(t) for t in tok[1:]]
        want = L + drift + A + x0
        assert len(got) == len(want) == d * (d + 1) + 2 * d
        assert [t.hex() for t in got] == [t.hex() for t in want], (d, kind, n_steps)
    for (Cm, reason), line in zip(INVALID, lines[len(VALID):]):
        assert line.startswith("invalid") and reason in line, (Cm, line)
        assert ac.corr_defect(Cm) is not None or ac.cholesky_fp64(Cm) is None
    assert re.search(rf"read {len(lines)} records; {len(INVALID)} invalid", run.stderr), run.stderr


@pytest.mark.parametrize("which", range(len(VALID)))
def test_the_factor_reproduces_the_matrix(which):
    """L·Lᵀ = C to a few ulp of 1 (exact products and sums of the fp64 factor, at 50 digits): 4 ulp per entry"""
    Cm = VALID[which][0]["corr"]
    d, L = len(Cm), ac.cholesky_fp64(Cm)
    with mp.workdps(50):
        for i in range(d):
            for j in range(i + 1):
                back = mp.fsum(mp.mpf(L[ac.tri(i, k)]) * mp.mpf(L[ac.tri(j, k)]) for k in range(j + 1))
                assert abs(back - mp.mpf(Cm[i][j])) <= 4 * 2.0 ** -52, (i, j)


# ---- closed forms -----------------------------------------------------------------------------------------------------------

def test_golden_file_is_what_its_maker_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_assets_exact", os.path.join(ROOT, "tests", "golden", "make_assets_exact.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert json.loads(json.dumps(mod.build())) == DOC


def test_golden_prices_are_the_issues_table():
    for (cid, name), (want, want0) in ac.ISSUE_TABLE.items():
        rec = DOC["prices"][cid][name]
        assert abs(float(rec["price"]) - want) < 6e-6 and abs(float(rec["rho0"]) - want0) < 6e-6, (cid, name)
    assert set(DOC["prices"]["e"]) == {"geometric_call_K100"}


def test_binormal_against_known_values():
    """Φ₂(0, 0; ρ) = ¼ + asin(ρ)/2π; ρ = 0 factorises"""
    with mp.workdps(50):
        for rho in (-0.7, 0.0, 0.3, 0.95):
            assert abs(ac.binormal(0, 0, rho) - (mp.mpf(1) / 4 + mp.asin(mp.mpf(rho)) / (2 * mp.pi))) < mp.mpf(10) ** -30
        assert abs(ac.binormal(0.3, -1.2, 0) - mp.ncdf(0.3) * mp.ncdf(-1.2)) < mp.mpf(10) ** -30


def _inputs(case):
    return hh.MultiAssetInputs(REF, case["r_drift"], case["spots"], case["sigmas"], case["corr"])


def _vanilla(K, cp=None):
    return hh.VanillaOption(K, EXP, hh.European(), cp or hh.Call(), hh.Spot())


def test_analytic_equals_the_golden_file():
    """MultiAssetAnalytic against both columns of the file, 1e-13 relative (2025 has 365 days: T = 1 exactly)"""
    from hedgehog_jl_amd.dates import yearfrac
    assert yearfrac(REF, EXP) == 1.0
    rows = [("a", "geometric_call_K100", hh.GeometricMean(ac.CASE_A["weights"]), 100.0, hh.Call()),
            ("a", "geometric_put_K105", hh.GeometricMean(ac.CASE_A["weights"]), 105.0, hh.Put()),
            ("e", "geometric_call_K100", hh.GeometricMean(ac.CASE_E["weights"]), 100.0, hh.Call()),
            ("b", "margrabe", hh.WeightedSum((1.0, -1.0)), 0.0, hh.Call())]
    for cid, name, index, K, cp in rows:
        for col, case in (("price", ac.CASES[cid]), ("rho0", ac.uncorrelated(ac.CASES[cid]))):
            got = hh.solve(hh.PricingProblem(hh.IndexOption(index, _vanilla(K, cp)), _inputs(case)), hh.MultiAssetAnalytic()).price
            assert got == pytest.approx(float(DOC["prices"][cid][name][col]), rel=1e-13), (cid, name, col)


def test_analytic_refuses_everything_else():
    inp = _inputs(ac.CASE_B)
    for opt in (hh.IndexOption(hh.WeightedSum((1.0, 1.0)), _vanilla(100.0)), hh.IndexOption(hh.WeightedSum((1.0, -1.0)), _vanilla(5.0)),
                hh.IndexOption(hh.WeightedSum((1.0, -1.0)), _vanilla(0.0, hh.Put())), hh.IndexOption(hh.BestOf(), _vanilla(100.0)),
                hh.IndexOption(hh.GeometricMean((0.5, 0.5)), hh.DigitalOption(100.0, EXP, hh.Call())), _vanilla(100.0)):
        with pytest.raises(hh.MethodError):
            hh.solve(hh.PricingProblem(opt, inp), hh.MultiAssetAnalytic())


# ---- the restatement's own sanity ----------------------------------------------------------------------------------------------

def test_restatement_in_floats_and_at_50_digits_agree():
    """two assets, three steps, fixed normals: the fp64 run is within 1e-13 relative of the 50-digit run on every row of
    every index kind, the mirror differs, and without volatility every date carries the index at the spots"""
    z = [[mp.mpf(t) for t in row] for row in ([0.3, -1.1], [0.0, 0.7], [-2.0, 0.4])]
    case = ac.path_case(2)
    for kind in ac.KINDS:
        ref = ac.path_reference(case, kind, [z], 1, 1, 1)
        for m in range(2):
            for row in range(5):
                assert ref["e64"][m, 0, row] <= 1e-13 * abs(float(ref["want"][m][0][row])), (kind, m, row)
        assert ref["want"][0][0][4] != ref["want"][1][0][4]
        still = ac.path_reference(dict(case, sigmas=[0.0, 0.0], r_drift=0.0), kind, [z], 0, 1, 1)
        I0 = ac.index_numpy(case, kind)
        assert float(still["want"][0][0][4]) == pytest.approx(I0, rel=1e-15)
        assert float(still["want"][0][0][0]) == pytest.approx(4 * I0, rel=1e-15)


# ---- the Python routes against a fake library ------------------------------------------------------------------------------------

class FakeLib:
    def __init__(self):
        self.calls = []

    def hh_seeds_fingerprint(self, ptr, n):
        return 1

    def hh_mc_solve_path_assets(self, handle, model, assets, cfg, every, start, payoffs, n, res, values, stats):
        a, m, c = assets._obj, model._obj, cfg._obj
        d = a.n_assets
        self.calls.append(dict(
            d=d, kind=a.index_kind, spots=list(a.spots[:d]), sigmas=list(a.sigmas[:d]), weights=list(a.weights[:d]),
            corr=[[a.corr[i * 8 + j] for j in range(d)] for i in range(d)], T=m.T, r=m.r_drift, D=m.discount,
            dynamics=c.dynamics, strategy=c.strategy, noise=c.noise_mode, partials=c.n_partials, anti=c.antithetic,
            n_paths=c.n_paths, n_steps=c.n_steps, every=every, start=start, stats=stats,
            payoffs=[(payoffs[k].kind, payoffs[k].strike, payoffs[k].cp, payoffs[k].barrier) for k in range(n)]))
        for k in range(n):
            res[k].price, res[k].std_error = 100.0 * len(self.calls) + k, 0.5
        return 0


class FakeCtx:
    handle = None

    def __init__(self):
        self.lib = FakeLib()

    def check(self, rc):
        assert rc == 0

    def seeds_on_device(self, seeds, fingerprint=0):
        return 4096


@pytest.fixture
def fake(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(_ffi, "get_context", lambda device=0: ctx)
    return ctx.lib


def _method(steps=6, n=16, vr=None, **kw):
    return hh.MonteCarlo(hh.MultiAssetDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(n, steps=steps, seeds=np.arange(n), variance_reduction=vr), **kw)


def test_a_single_solve_packs_the_call(fake):
    inp = _inputs(ac.CASE_A)
    opt = hh.IndexOption(hh.WeightedSum(ac.CASE_A["weights"]), hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2, True)))
    sol = hh.solve(hh.PricingProblem(opt, inp), _method(vr=hh.Antithetic()))
    (call,) = fake.calls
    assert isinstance(sol, hh.MonteCarloSolution) and sol.price == 100.0 and sol.std_error == 0.5
    assert sol.ensemble.shape == (5, 32) and call["stats"] == sol.ensemble.ctypes.data
    assert (call["d"], call["kind"], call["spots"], call["sigmas"], call["weights"]) == \
        (3, ac.SUM, ac.CASE_A["spots"], ac.CASE_A["sigmas"], ac.CASE_A["weights"])
    assert call["corr"] == ac.CASE_A["corr"]
    assert (call["dynamics"], call["strategy"], call["noise"], call["partials"], call["anti"]) == (ac.GBM, ac.EULER, 0, 0, 1)
    assert (call["n_paths"], call["n_steps"], call["every"], call["start"]) == (16, 6, 2, 1)
    assert call["r"] == 0.03 and call["D"] == pytest.approx(math.exp(-0.03 * call["T"]), rel=1e-15) and call["T"] == 1.0
    assert call["payoffs"] == [(_ffi.HH_PAYOFF_ASIAN_ARITH, 100.0, 1.0, 0.0)]
    # a payoff that reads expiry alone is monitored at expiry; BestOf() has unit weights
    hh.solve(hh.PricingProblem(hh.IndexOption(hh.BestOf(), _vanilla(90.0, hh.Put())), inp), _method(), ensemble=False)
    call = fake.calls[1]
    assert (call["every"], call["start"], call["kind"], call["weights"], call["stats"]) == (6, 0, ac.BEST, [1.0, 1.0, 1.0], None)
    assert call["payoffs"] == [(_ffi.HH_PAYOFF_VANILLA, 90.0, -1.0, 0.0)]


def test_a_basket_takes_one_pass_per_index(fake):
    inp = _inputs(ac.CASE_A)
    w = ac.CASE_A["weights"]
    basket, worst, mon = hh.WeightedSum(w), hh.WorstOf(), hh.Monitoring(1, False)
    opts = [hh.IndexOption(basket, _vanilla(100.0)),
            hh.IndexOption(worst, _vanilla(95.0, hh.Put())),
            hh.IndexOption(hh.WeightedSum(tuple(w)), hh.AsianOption(100.0, EXP, hh.Call(), monitoring=mon)),
            hh.IndexOption(basket, hh.BarrierOption(100.0, 130.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=mon)),
            hh.IndexOption(hh.WeightedSum((1.0, -1.0, 0.0)), _vanilla(5.0))]
    out = hh.solve(hh.BasketPricingProblem(opts, inp), _method())
    assert [c["kind"] for c in fake.calls] == [ac.SUM, ac.WORST, ac.SUM]
    assert [k for k, *_ in fake.calls[0]["payoffs"]] == [_ffi.HH_PAYOFF_VANILLA, _ffi.HH_PAYOFF_ASIAN_ARITH, _ffi.HH_PAYOFF_BARRIER]
    assert (fake.calls[0]["every"], fake.calls[0]["start"]) == (1, 0) and fake.calls[2]["weights"] == [1.0, -1.0, 0.0]
    assert [s.price for s in out.solutions] == [100.0, 200.0, 101.0, 102.0, 300.0]
    assert [s.problem.payoff for s in out.solutions] == opts
    # two monitorings of one index: two passes
    fake.calls.clear()
    other = hh.IndexOption(basket, hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(3, True)))
    hh.solve(hh.BasketPricingProblem([opts[2], other], inp), _method())
    assert [(c["every"], c["start"]) for c in fake.calls] == [(1, 0), (3, 1)]


def test_refusals_touch_no_device(fake):
    inp, bs = _inputs(ac.CASE_B), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    opt = hh.IndexOption(hh.WeightedSum((1.0, 1.0)), _vanilla(100.0))
    gbm = hh.MonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(8, steps=2, seeds=np.arange(8)))
    american = hh.IndexOption(hh.BestOf(), hh.VanillaOption(100.0, EXP, hh.American(), hh.Put(), hh.Spot()))
    cont = hh.IndexOption(hh.BestOf(), hh.BarrierOption(100.0, 150.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=hh.ContinuousMonitoring()))
    exact = hh.MonteCarlo(hh.MultiAssetDynamics(), hh.BlackScholesExact(), hh.SimulationConfig(8, seeds=np.arange(8)))
    cases = [
        (hh.PricingProblem(opt, bs), _method()), (hh.PricingProblem(opt, inp), gbm), (hh.PricingProblem(opt, bs), gbm),
        (hh.PricingProblem(opt, inp), exact),
        (hh.PricingProblem(_vanilla(100.0), inp), _method()),
        (hh.PricingProblem(hh.AsianOption(100.0, EXP, hh.Call()), inp), _method()),
        (hh.PricingProblem(cont, inp), _method()), (hh.PricingProblem(american, inp), _method()),
        (hh.PricingProblem(opt, inp), _method(devices=range(2))),
        (hh.PricingProblem(opt, inp), hh.LSM(hh.LognormalDynamics(), hh.BlackScholesExact(), hh.SimulationConfig(8, seeds=np.arange(8)), 3)),
        (hh.PricingProblem(opt, inp), hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics())),
        (hh.PricingProblem(opt, inp), hh.CoxRossRubinsteinMethod(10)),
        (hh.PricingProblem(opt, inp), hh.CrankNicolsonMethod(20, 20)),
        (hh.PricingProblem(opt, inp), hh.BlackScholesAnalytic()),
        (hh.BasketPricingProblem([opt, _vanilla(100.0)], inp), _method()),
        (hh.BasketPricingProblem([opt], inp), hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics())),
        (hh.PricingProblem(hh.IndexOption(hh.WeightedSum((1.0, -1.0)), hh.AsianOption(1.0, EXP, hh.Call(), hh.GeometricAverage())), inp), _method()),
    ]
    for prob, method in cases:
        with pytest.raises(hh.MethodError):
            hh.solve(prob, method)
    with pytest.raises(hh.MethodError, match="no replay"):
        hh.solve(hh.PricingProblem(opt, inp), _method(), replay=np.zeros((8, 6, 1)))
    # a Dual anywhere in the inputs, and ForwardAD: the text names FiniteDifference
    dual = hh.Dual(100.0, (1.0,))
    for m in (inp.replace(spots=(dual, 95.0)), inp.replace(sigmas=(0.3, hh.Dual(0.25, (1.0,)))),
              hh.MultiAssetInputs(REF, hh.Dual(0.03, (1.0,)), *[ac.CASE_B[k] for k in ("spots", "sigmas", "corr")])):
        with pytest.raises(hh.MethodError, match="FiniteDifference"):
            hh.solve(hh.PricingProblem(opt, m), _method())
    for lens in (hh.AssetSpotLens(0), hh.AssetVolLens(1), hh.CorrelationLens(0, 1)):
        with pytest.raises(hh.MethodError, match="FiniteDifference"):
            hh.solve(hh.GreekProblem(hh.PricingProblem(opt, inp), lens), hh.ForwardAD(), _method())
    assert fake.calls == []


def test_value_errors(fake):
    inp = _inputs(ac.CASE_A)
    with pytest.raises(ValueError, match="divide"):
        hh.solve(hh.PricingProblem(hh.IndexOption(hh.BestOf(), hh.AsianOption(1.0, EXP, hh.Call(), monitoring=hh.Monitoring(4))), inp), _method())
    with pytest.raises(ValueError, match="2 weights for 3 assets"):
        hh.solve(hh.PricingProblem(hh.IndexOption(hh.WeightedSum((1.0, 1.0)), _vanilla(1.0)), inp), _method())
    assert fake.calls == []
    ok = ac.CASE_B
    for kw, text in ((dict(spots=[100.0, -1.0]), "spot"), (dict(spots=[100.0, float("inf")]), "spot"), (dict(sigmas=[0.2, -0.1]), "sigma"),
                     (dict(sigmas=[0.2]), "2 sigmas"), (dict(corr=[[1.0, 0.5], [0.4, 1.0]]), "symmetric"),
                     (dict(corr=[[1.0, 0.5], [0.5, 0.9]]), "diagonal"), (dict(corr=[[1.0, 1.0], [1.0, 1.0]]), "positive definite"),
                     (dict(corr=[[1.0, 1.5], [1.5, 1.0]]), r"\[-1, 1\]"), (dict(corr=[[1.0, NAN], [NAN, 1.0]]), "finite"),
                     (dict(spots=[1.0] * 9, sigmas=[0.1] * 9, corr=ac.decay_corr(9)), "assets"), (dict(spots=[], sigmas=[], corr=[]), "assets")):
        with pytest.raises(ValueError, match=text):
            _inputs(dict(ok, **kw))
    for make in (lambda: hh.WeightedSum((0.0, 0.0)), lambda: hh.WeightedSum((1.0, NAN)), lambda: hh.BestOf((1.0, 0.0)),
                 lambda: hh.WorstOf((1.0, -1.0)), lambda: hh.GeometricMean(()), lambda: hh.GeometricMean((float("inf"),))):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(TypeError):
        hh.IndexOption(hh.BestOf(), 3.0)
    with pytest.raises(TypeError):
        hh.IndexOption("basket", _vanilla(1.0))


def test_lenses_through_set_and_finite_differences(fake):
    inp = _inputs(ac.CASE_A)
    prob = hh.PricingProblem(hh.IndexOption(hh.GeometricMean(ac.CASE_A["weights"]), _vanilla(100.0)), inp)
    assert (hh.AssetSpotLens(1)(prob), hh.AssetVolLens(2)(prob), hh.CorrelationLens(0, 2)(prob)) == (90.0, 0.25, -0.3)
    p = hh.set(prob, hh.AssetSpotLens(1), 91.0)
    assert p.market_inputs.spots == (100.0, 91.0, 110.0) and prob.market_inputs.spots == (100.0, 90.0, 110.0)
    p = hh.set(prob, hh.AssetVolLens(2), 0.3)
    assert p.market_inputs.sigmas == (0.2, 0.35, 0.3) and p.payoff == prob.payoff
    p = hh.set(prob, hh.CorrelationLens(0, 2), 0.1)
    assert p.market_inputs.correlation[0][2] == p.market_inputs.correlation[2][0] == 0.1
    assert p.market_inputs.correlation[0][1] == 0.6
    with pytest.raises(ValueError, match="positive definite"):
        hh.set(prob, hh.CorrelationLens(0, 2), -0.99)
    with pytest.raises(ValueError):
        hh.CorrelationLens(1, 1)
    with pytest.raises(TypeError):
        hh.AssetSpotLens(0)(hh.PricingProblem(_vanilla(1.0), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)))
    # a central difference: two plain solves, one after the other, on the bumped spot
    g = hh.solve(hh.GreekProblem(prob, hh.AssetSpotLens(0)), hh.FiniteDifference(1e-2), _method())
    assert [c["spots"][0] for c in fake.calls] == [101.0, 99.0] and g.greek == pytest.approx((100.0 - 200.0) / 2.0)
    assert hh.solve_montecarlo_many([prob, prob], _method()) is None
