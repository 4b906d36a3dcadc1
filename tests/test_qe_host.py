"""Heston paths by the quadratic-exponential scheme on the host side, without a GPU: the struct and the two entry points
declared, exported and bound; the step of csrc/hh_qe.h as a stand-alone host program (also under AddressSanitizer and
UBSan) against the Python-float restatement, bit for bit, and against long double inside the program; the restatement's
own point — the conditional mean and variance of v′ and, with the correction, the martingale identity — by exact
integration at 50 digits; the fixture's conditions and its maker; the mutations of the restatement against the golden
rows; how the Python layer routes and refuses."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from hedgehog_jl_amd import montecarlo as hmc  # noqa: E402
from hedgehog_jl_amd import routes  # noqa: E402
from tests import oracle_ffi  # noqa: E402
from tests import qe_cases as qc  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_qe": 10, "hh_mc_solve_path_qe": 12}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2026, 1, 1)
DOC = qc.load_golden()


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
    assert re.search(r"HH_BROADIE_KAYA = 2,\s*HH_QE = 3\b", hdr) and _ffi.HH_QE == 3
    assert (_ffi.HH_EULER_MARUYAMA, _ffi.HH_EXACT_LAW, _ffi.HH_BROADIE_KAYA) == (0, 1, 2)  # no existing value changes
    assert re.search(r"#define HH_QE_MAX_PSI\s+1e9\b", hdr) and _ffi.HH_QE_MAX_PSI == 1e9
    assert "hh_qe.hip" in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "kDomQe = 5u" in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_rng.h")).read() and qc.DOM_QE == 5
    assert "#include <hip" not in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_qe.h")).read()  # a host program includes it


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_hh_qe_layout(tmp_path):
    """hh_qe is 16 bytes — a double at 0, two int32 at 8 and 12: a compiled offsetof dump against the ctypes structure"""
    fields = ["psi_c", "martingale", "reserved"]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(hh_qe));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(hh_qe, {f}), sizeof(((hh_qe*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, env=host_env()).stdout.split("\n")
    assert out[0] == "sizeof 16" and C.sizeof(_ffi.hh_qe) == 16
    got = [(n, getattr(_ffi.hh_qe, n).offset, getattr(_ffi.hh_qe, n).size) for n, _ in _ffi.hh_qe._fields_]
    want = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:4]]
    assert got == want == [("psi_c", 0, 8), ("martingale", 8, 4), ("reserved", 12, 4)]
    q = _ffi.make_qe(1.25, True)
    assert (q.psi_c, q.martingale, q.reserved) == (1.25, 1, 0)


# ---- the step as a host program ------------------------------------------------------------------------------------------

def sweep():
    """(model, psi_c, dt, v, x, zv, zx, U, mart): states on both sides of ψ_c for every model and ψ_c, both arms of U"""
    rng = np.random.default_rng(20261019)
    rows = []
    for case in (qc.MODELS["feller"], qc.MODELS["low_v0"], qc.DRIFTY, dict(qc.LAW, rho=0.6)):
        for psi_c in (0.0, 1.0, 1.25, 2.0):
            for dt in (1.0 / 252, 1.0 / 12, 0.3125, 1.25):
                for v in (0.0, 1e-6, 1e-3, 0.02, 0.04, 0.3, 2.0):
                    for _ in range(2):
                        mart = int(rng.integers(0, 2)) if case["rho"] <= 0 else 0
                        rows.append((case, psi_c, dt, v, float(rng.normal(4.6, 0.3)), float(rng.normal()), float(rng.normal()),
                                     bc_u01(rng), mart))
    return rows


def bc_u01(rng):
    """a uniform the device can draw: (k + ½)·2⁻⁵², k of 52 bits"""
    return (int(rng.integers(0, 2 ** 52)) + 0.5) * 2.0 ** -52


def restated_step(case, psi_c, dt, v, x, zv, zx, U, mart):
    """tests/qe_cases.step in Python floats on one state -> (branch, v′, x′)"""
    q = qc.constants(dict(case, T=dt), 1, float, psi_c)
    rec = []
    xn, vn = qc.step(q, qc.VA(x), qc.VA(v), qc.VA(zv), qc.VA(zx), qc.VA(U), mart, float, rec)
    _, quad, zero, _ = rec[0]
    return (0 if quad else 2 if zero else 1), vn.v, xn.v


def _build_host_check(tmp_path, flags, name):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "qe_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_step_host_program(tmp_path, build):
    """tests/c/qe_host_check.cpp — its own main, csrc/hh_qe.h included — takes the step of every state of the sweep:
    its v′ and x′ are the Python-float restatement's, bit for bit (the same IEEE operations in the same order), its
    branches the restatement's, and inside the program every step lies within 1e-13 of a long-double evaluation.  Built
    plainly and with -fsanitize=address,undefined, and run as a program: nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = _build_host_check(tmp_path, flags, "qe_host_check_" + build)
    rows = sweep()
    with open(tmp_path / "rows.txt", "w") as f:
        for case, psi_c, dt, v, x, zv, zx, U, mart in rows:
            nums = [case["kappa"], case["theta"], case["sigma"], case["rho"], case["r_drift"], dt, psi_c, v, x, zv, zx, U]
            f.write(" ".join(float(t).hex() for t in nums) + f" {mart}\n")
    run = subprocess.run([exe, str(tmp_path / "rows.txt")], capture_output=True, text=True, env=host_env(), timeout=120)
    assert run.returncode == 0, run.stderr
    got = [ln.split() for ln in run.stdout.splitlines()]
    assert len(got) == len(rows)
    seen = set()
    for row, (branch, vn, xn) in zip(rows, got):
        want = restated_step(*row)
        assert (int(branch), float.fromhex(vn), float.fromhex(xn)) == want, (row, branch, vn, xn, want)
        seen.add(int(branch))
    assert seen == {0, 1, 2}
    assert re.search(r"compared [1-9]\d* quadratic, [1-9]\d* exponential steps; 0 bad", run.stderr), run.stderr


# ---- the point of the scheme: moments and the martingale identity, by exact integration ----------------------------------

STATES = [("feller", 5, 0.04), ("feller", 5, 0.0), ("feller", 1, 0.5), ("low_v0", 6, 0.001), ("low_v0", 6, 0.9),
          ("low_v0", 16, 0.0), ("drifty", 8, 0.04), ("drifty", 8, 3.0)]


def _case(name):
    return qc.DRIFTY if name == "drifty" else qc.MODELS[name]


def test_variance_step_matches_the_conditional_mean_and_variance():
    """E v′ = m and Var v′ = s² in both branches, integrating the restatement's own v′ over Z_v (quadratic) or over the
    atom and the density of U's inverse (exponential): to 1e-30.  m and s² against the CIR closed forms too."""
    branches = set()
    with mp.workdps(qc.DPS):
        for name, n_steps, v in STATES:
            case = _case(name)
            mean, branch, m, psi = qc.step_expectation(case, n_steps, v, lambda vn, d, w: vn)
            second, _, _, _ = qc.step_expectation(case, n_steps, v, lambda vn, d, w: vn * vn)
            s2 = psi * m * m
            assert abs(mean - m) < mp.mpf(10) ** -30 and abs(second - mean * mean - s2) < mp.mpf(10) ** -30, (name, n_steps, v, branch)
            k, th, sg = (mp.mpf(case[t]) for t in ("kappa", "theta", "sigma"))
            dt = mp.mpf(case["T"]) / n_steps
            E = mp.exp(-k * dt)
            assert abs(m - (th + (mp.mpf(v) - th) * E)) < mp.mpf(10) ** -40
            assert abs(s2 - (mp.mpf(v) * sg ** 2 * E * (1 - E) / k + th * sg ** 2 * (1 - E) ** 2 / (2 * k))) < mp.mpf(10) ** -40
            branches.add(branch)
    assert branches == {"quadratic", "exponential"}


def test_the_correction_makes_the_step_a_martingale():
    """E exp(K0* + K1·v + K2·v′ + ½(K3·v + K4·v′)) = 1 in both branches, to 1e-30; without the correction it is not; the
    mutation K3 for K3/2 breaks it"""
    f = lambda vn, drift, var: mp.exp(drift + var / 2)  # noqa: E731
    branches = set()
    with mp.workdps(qc.DPS):
        for name, n_steps, v in STATES:
            got, branch, _, _ = qc.step_expectation(_case(name), n_steps, v, f, mart=True)
            assert abs(got - 1) < mp.mpf(10) ** -30, (name, n_steps, v, branch, got)
            branches.add(branch)
        plain, _, _, _ = qc.step_expectation(qc.DRIFTY, 8, 0.04, f, mart=False)
        assert abs(plain - 1) > mp.mpf(10) ** -4
        wrong, _, _, _ = qc.step_expectation(qc.DRIFTY, 8, 0.04, f, mart=True, mut="K3_full")
        assert abs(wrong - 1) > mp.mpf(10) ** -4
    assert branches == {"quadratic", "exponential"}


# ---- the fixture -----------------------------------------------------------------------------------------------------------

def test_maker_regenerates_the_fixture_identically():
    """the maker runs on the CPU; it asserts equal branches in both precisions and the margin on every trajectory"""
    spec = importlib.util.spec_from_file_location("make_qe_exact", os.path.join(ROOT, "tests", "golden", "make_qe_exact.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    again = json.loads(json.dumps(maker.build(oracle_ffi.load())))
    assert again == DOC
    assert DOC["margin"] == qc.MARGIN == 1e-9 and DOC["n_paths"] == qc.PATH_N == 257
    assert {(b["model"], b["n_steps"]) for b in DOC["branches"]} == {(m, s) for m in qc.MODELS for s, _ in qc.PATH_SHAPES}
    for b in DOC["branches"]:
        assert b["quadratic"] + b["exponential"] == 2 * qc.PATH_N * b["n_steps"]
        if b["n_steps"] > 1:
            assert b["quadratic"] > 0 and b["exponential"] > b["zero"] > 0, b
    by = {(b["model"], b["n_steps"]): b for b in DOC["branches"]}
    assert by[("feller", 5)]["quadratic"] > by[("feller", 5)]["exponential"]   # mostly below ψ_c
    assert by[("low_v0", 5)]["quadratic"] < by[("low_v0", 5)]["exponential"]   # mostly above


# ---- mutations of the restatement against the golden rows ----------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_draws():
    oracle, seeds, n_steps = oracle_ffi.load(), qc.path_seeds()[:qc.GOLDEN_N], qc.GOLDEN_SHAPE[0]
    return qc.step_normals(oracle, seeds, n_steps), qc.step_uniforms(oracle, seeds, n_steps)


def misses(rec, golden_draws, mut):
    """per member: how many (path, row) of the fp64 restatement — mutated by `mut` — lie outside the golden bars"""
    Z, U = golden_draws
    case, n_steps, every = qc.MODELS[rec["model"]], *qc.GOLDEN_SHAPE
    out = [0, 0]
    with mp.workdps(qc.DPS):
        for m in range(2):
            for i in range(qc.GOLDEN_N):
                Z64 = [(float(a), float(b)) for a, b in Z[i]]
                xs, vT = qc.walk(case, n_steps, float, Z64, U[i], m == 1, rec["martingale"], None, mut)
                got = qc.rows_of(case, xs, float, every, 0) + [vT]
                for row in range(6):
                    if abs(mp.mpf(got[row].v) - mp.mpf(rec["want"][m][i][row])) > rec["bars"][m][i][row]:
                        out[m] += 1
    return out


def test_mutations_move_the_restatement_beyond_the_bars(golden_draws):
    """The golden rows are those of the device's path test (the same walk, seeds and bars).  Unmutated, the fp64
    restatement is inside every bar; K1 <-> K2 and b for b² in a move both models, p = (ψ − 1)/ψ the model that lives in
    the exponential branch (and the other one's visits to it), a mirror that keeps U the mirrors only, K3 for K3/2 the
    corrected runs only."""
    recs = {(r["model"], r["martingale"]): r for r in DOC["rows"]}
    assert set(recs) == {(m, k) for m in qc.MODELS for k in (0, 1)}
    for key, rec in recs.items():
        assert misses(rec, golden_draws, None) == [0, 0], key
        found = {mut: misses(rec, golden_draws, mut) for mut in qc.MUTATIONS}
        print(f"\n{key}: (path, row) pairs outside the bars, [trajectories, mirrors], of {6 * qc.GOLDEN_N} each: {found}")
        assert min(found["swap_K"]) > 0 and min(found["b_not_b2"]) > 0 and min(found["p_over_psi"]) > 0, (key, found)
        assert found["keep_U"][0] == 0 and found["keep_U"][1] > 0, (key, found)
        assert (min(found["K3_full"]) > 0) if key[1] else (found["K3_full"] == [0, 0]), (key, found)


# ---- routing ---------------------------------------------------------------------------------------------------------------

def heston_inputs(**kw):
    c = dict(qc.LAW, **kw)
    return hh.HestonInputs(REF, c["r_drift"], c["S0"], c["V0"], c["kappa"], c["theta"], c["sigma"], c["rho"])


def vanilla(K=100.0, style=None):
    return hh.VanillaOption(K, EXP, style or hh.European(), hh.Call(), hh.Spot())


def _mc(dyn, strat, steps=4, n=8, **kw):
    return hh.MonteCarlo(dyn, strat, hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64)), **kw)


def test_strategy_and_structs():
    s = hh.HestonQE()
    assert (s.psi_c, s.martingale) == (1.5, False) and hh.HestonQE(2.0, True) == hh.HestonQE(psi_c=2.0, martingale=True)
    assert isinstance(s, hmc.SimulationStrategy) and "HestonQE" in hh.solve.__doc__
    for bad in (0.0, 0.99, 2.01, float("nan")):
        with pytest.raises(ValueError, match=r"psi_c must lie in \[1, 2\]"):
            hh.HestonQE(psi_c=bad)
    curve = hh.RateCurve(REF, [0.5, 6.0], zeros=[0.01, 0.04])
    mkt = hh.HestonInputs(REF, curve, 100.0, 0.04, 0.3, 0.04, 0.9, -0.5)
    model, c, (q,) = routes.QE.form_structs(vanilla(), mkt, _mc(hh.HestonDynamics(), hh.HestonQE(1.25, True), steps=12))
    assert (c.dynamics, c.strategy, c.n_steps, c.n_partials, c.antithetic) == (_ffi.HH_HESTON, _ffi.HH_QE, 12, 0, 0)
    assert model.r_drift == hh.zero_rate(curve, 0.0) and model.T == hh.yearfrac(REF, EXP) and model.discount == hh.df(curve, EXP)
    assert (model.V0, model.kappa, model.theta, model.sigma, model.rho) == (0.04, 0.3, 0.04, 0.9, -0.5)
    assert (q.psi_c, q.martingale, q.reserved) == (1.25, 1, 0)


def test_method_errors_name_the_alternative():
    hi, bs = heston_inputs(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    qe = _mc(hh.HestonDynamics(), hh.HestonQE())
    refused = [
        (vanilla(), bs, _mc(hh.LognormalDynamics(), hh.HestonQE()), "EulerMaruyama"),
        (vanilla(), bs, qe, "HestonInputs"),
        (vanilla(), hi, _mc(hh.LognormalDynamics(), hh.HestonQE()), "HestonDynamics"),
        (vanilla(), hi, _mc(hh.HestonDynamics(), hh.HestonQE(), devices=(0,)), "one device"),
        (vanilla(style=hh.American()), hi, qe, "LSM"),
        (hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.ContinuousMonitoring()), hi, qe, "EulerMaruyama()"),
        (hh.LookbackOption(EXP, hh.Call(), monitoring=hh.ContinuousMonitoring()), hi, qe, "Monitoring"),
        (vanilla(), heston_inputs(S0=hh.Dual(100.0, (1.0,))), qe, "FiniteDifference"),
    ]
    for payoff, mkt, method, text in refused:
        with pytest.raises(hh.MethodError, match=re.escape(text)):
            hh.solve(hh.PricingProblem(payoff, mkt), method)
    with pytest.raises(hh.MethodError, match="replay"):
        hh.solve(hh.PricingProblem(vanilla(), hi), qe, replay=np.zeros(8))
    with pytest.raises(hh.MethodError, match="FiniteDifference"):  # ForwardAD: no partials are carried
        hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla(), hi), hh.SpotLens()), hh.ForwardAD(), qe)
    assert hmc.solve_montecarlo_many([hh.PricingProblem(vanilla(), hi)] * 2, qe) is None  # plain solves, one by one


def test_basket_groups_share_one_simulation(monkeypatch):
    from hedgehog_jl_amd import basket as hb
    hi = heston_inputs()
    later = hh.Date(2027, 1, 1)
    payoffs = [hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2)), vanilla(95.0),
               hh.DigitalOption(101.0, EXP, hh.Put()), hh.VanillaOption(110.0, later, hh.European(), hh.Put(), hh.Spot()),
               hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(2))]
    calls = []

    def fake_paths(group, market_inputs, method, ensemble=True, route=None):
        calls.append([payoffs.index(p) if p in payoffs else p.strike for p in group])
        return [hh.MonteCarloSolution(hh.PricingProblem(p, market_inputs), method, 0.0) for p in group]

    monkeypatch.setattr(hb, "solve_path_payoffs", fake_paths)
    sol = hh.solve(hh.BasketPricingProblem(payoffs, hi), _mc(hh.HestonDynamics(), hh.HestonQE()))
    assert calls == [[0, 1, 2, 4], [3]] and all(s is not None for s in sol.solutions)
    calls.clear()
    hh.solve(hh.BasketPricingProblem([vanilla(96.0), vanilla(106.0)], hi), _mc(hh.HestonDynamics(), hh.HestonQE()))
    assert calls == [[96.0, 106.0]]  # European vanillas alone: the vanilla kind, monitored at expiry
