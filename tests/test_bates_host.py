"""Bates — Heston QE paths with Merton jumps — on the host side, without a GPU: the three entry points declared, exported
and bound; the step composed from csrc/hh_qe.h and csrc/hh_jump.h as a stand-alone host program (also under
AddressSanitizer and UBSan) against the Python-float restatement, bit for bit; the restatement's own point — with the
correction the step is a martingale, jumps included — by exact integration at 50 digits; the fixture's conditions and its
maker; the mutations of the restatement against the golden rows; the numpy restatement of the Carr–Madan rule against the
exactly integrated truncated integral; how the Python layer routes and refuses."""
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
from tests import bates_cases as bt  # noqa: E402
from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import merton_cases as mc  # noqa: E402
from tests import oracle_ffi  # noqa: E402
from tests import qe_cases as qc  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_path_stats_bates": 11, "hh_mc_solve_path_bates": 13, "hh_carr_madan_bates": 12}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2026, 1, 1)
DOC = bt.load_golden()


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
    assert (_ffi.HH_LOGNORMAL, _ffi.HH_HESTON, _ffi.HH_QE) == (0, 1, 3)  # no enum gains a value
    assert (C.sizeof(_ffi.hh_qe), C.sizeof(_ffi.hh_jump)) == (16, 24)     # no struct changes size
    assert '"hh_bates.hip"' in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    for h in ("hh_qe.h", "hh_jump.h"):  # a host program includes them
        assert "#include <hip" not in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", h)).read()


# ---- the step as a host program ------------------------------------------------------------------------------------------

def sweep():
    """(case, psi_c, dt, v, x, zv, zx, U, UJ, z, mart, mirror): a few hundred states on both sides of ψ_c, both arms of U,
    jump uniforms that reach every N of 0 … 4 and beyond, both members"""
    rng = np.random.default_rng(19960101)
    u01 = lambda: (int(rng.integers(0, 2 ** 52)) + 0.5) * 2.0 ** -52  # noqa: E731 - a uniform the device can draw
    jumps = (dict(lam=0.9, mu_j=-0.1, sigma_j=0.15), dict(lam=4.0, mu_j=0.05, sigma_j=0.0), dict(lam=0.0, mu_j=-0.1, sigma_j=0.15))
    rows = []
    for case in (qc.MODELS["feller"], qc.MODELS["low_v0"], qc.DRIFTY, dict(qc.LAW, rho=0.6)):
        for jump in jumps:
            for psi_c in (0.0, 1.25):
                for dt in (1.0 / 252, 0.3125, 1.0):
                    for v in (0.0, 1e-3, 0.04, 0.3, 2.0):
                        mart = int(rng.integers(0, 2)) if case["rho"] <= 0 else 0
                        UJ = u01() if rng.integers(0, 3) else 1.0 - 2.0 ** -12 * u01()  # a third in the far tail
                        rows.append((dict(case, **jump), psi_c, dt, v, float(rng.normal(4.6, 0.3)), float(rng.normal()),
                                     float(rng.normal()), u01(), UJ, float(rng.normal()), mart, int(rng.integers(0, 2))))
    return rows


def restated_step(case, psi_c, dt, v, x, zv, zx, U, UJ, z, mart, mirror):
    """one step of tests/bates_cases.walk in Python floats on one state -> (branch, N, v′, x′)"""
    one = dict(case, T=dt, S0=1.0, V0=v)
    N = mc.poisson_fp64(UJ, bt.path_mean(one, 1))
    q = bt.constants(one, 1, float, psi_c)
    rec = []
    a, b, u, zz = qc.VA(zv), qc.VA(zx), qc.VA(U), qc.VA(z)
    if mirror:
        a, b, u, zz = -a, -b, q["one"] - u, -zz
    xn, vn = qc.step(q, qc.VA(x), qc.VA(v), a, b, u, mart, float, rec)
    if N > 0:
        xn = xn + bt.jump_of(one, N, zz, float)
    _, quad, zero, _ = rec[0]
    return (0 if quad else 2 if zero else 1), N, vn.v, xn.v


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_step_host_program(tmp_path, build):
    """tests/c/bates_host_check.cpp — its own main, csrc/hh_qe.h and csrc/hh_jump.h included — takes the step of every
    state of the sweep: its branch, N, v′ and x′ are the Python-float restatement's, bit for bit (the same IEEE
    operations in the same order; the jump sum one fma).  Built plainly and with -fsanitize=address,undefined, and run as
    a program: nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = tmp_path / ("bates_host_check_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "bates_host_check.cpp"), "-o", str(exe)], check=True)
    rows = sweep()
    assert 300 <= len(rows) <= 1000
    with open(tmp_path / "rows.txt", "w") as f:
        for case, psi_c, dt, v, x, zv, zx, U, UJ, z, mart, mirror in rows:
            nums = [case["kappa"], case["theta"], case["sigma"], case["rho"], case["r_drift"], dt, psi_c, case["lam"],
                    case["mu_j"], case["sigma_j"], v, x, zv, zx, U, UJ, z]
            f.write(" ".join(float(t).hex() for t in nums) + f" {mart} {mirror}\n")
    run = subprocess.run([str(exe), str(tmp_path / "rows.txt")], capture_output=True, text=True, env=host_env(), timeout=120)
    assert run.returncode == 0, run.stderr
    got = [ln.split() for ln in run.stdout.splitlines()]
    assert len(got) == len(rows)
    seen_b, seen_n = set(), set()
    for row, (branch, N, vn, xn) in zip(rows, got):
        want = restated_step(*row)
        assert (int(branch), int(N), float.fromhex(vn), float.fromhex(xn)) == want, (row, branch, N, vn, xn, want)
        seen_b.add(int(branch))
        seen_n.add(int(N))
    assert seen_b == {0, 1, 2} and {0, 1, 2, 3, 4} <= seen_n
    assert re.search(r"stepped [1-9]\d* rows; 0 bad", run.stderr), run.stderr


# ---- the point of the compensator: one step is a martingale ----------------------------------------------------------------

STATES = [("feller", 5, 0.04), ("feller", 5, 0.0), ("low_v0", 6, 0.001), ("low_v0", 6, 0.9), ("drifty", 8, 0.04), ("drifty", 8, 3.0)]


def _case(name, n_steps):
    base = qc.DRIFTY if name == "drifty" else qc.MODELS[name]
    return dict(base, lam=bt.PATH_MEAN * n_steps / base["T"], **bt.JUMP)


def test_one_step_is_a_martingale_with_the_correction():
    """E exp(x′ − x − r·dt) = 1 to 1e-25 in both branches: qe_cases.step_expectation's integral over the variance step
    (Z_x in closed form) with r_c for r, times the Poisson-normal sum of the jump.  r or r + λκ̄ in place of r_c miss by
    exp(±λκ̄·dt); without the correction the QE part alone misses."""
    branches = set()
    with mp.workdps(qc.DPS):
        for name, n_steps, v in STATES:
            case = _case(name, n_steps)
            got, branch = bt.step_expectation(case, n_steps, v, mart=True)
            assert abs(got - 1) < mp.mpf(10) ** -25, (name, n_steps, v, branch, got)
            branches.add(branch)
            for mut in ("r_plain", "r_plus"):
                wrong, _ = bt.step_expectation(case, n_steps, v, mart=True, mut=mut)
                assert abs(wrong - 1) > mp.mpf(10) ** -3, (name, mut, wrong)
        plain, _ = bt.step_expectation(_case("drifty", 8), 8, 0.04, mart=False)
        assert abs(plain - 1) > mp.mpf(10) ** -4
    assert branches == {"quadratic", "exponential"}


# ---- the fixture -----------------------------------------------------------------------------------------------------------

def test_maker_regenerates_the_fixture_identically():
    """the maker runs on the CPU; it asserts equal branches in both precisions, the margins of ψ, U and every jump uniform
    on every trajectory, and that a case of more than one step sees both branches and an N >= 2"""
    spec = importlib.util.spec_from_file_location("make_bates_exact", os.path.join(ROOT, "tests", "golden", "make_bates_exact.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    again = json.loads(json.dumps(maker.build(oracle_ffi.load())))
    assert again == DOC
    assert DOC["margin"] == qc.MARGIN == mc.MARGIN == 1e-9 and DOC["n_paths"] == bt.PATH_N == 257
    assert bt.PATH_SHAPES == ((1, 1), (5, 1), (6, 1), (6, 3))
    assert {(b["model"], b["n_steps"]) for b in DOC["seen"]} == {(m, s) for m in bt.MODELS for s, _ in bt.PATH_SHAPES}
    for b in DOC["seen"]:
        assert b["quadratic"] + b["exponential"] == 2 * bt.PATH_N * b["n_steps"] == sum(b["N"].values())
        if b["n_steps"] > 1:
            assert b["quadratic"] > 0 and b["exponential"] > 0 and max(map(int, b["N"])) >= 2, b
    assert set(DOC["carr_madan"]) == set(bt.CM_CASES)


# ---- mutations of the restatement against the golden rows ----------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_draws():
    return bt.draws(oracle_ffi.load(), bt.path_seeds()[:bt.GOLDEN_N], bt.GOLDEN_SHAPE[0])


def misses(rec, d, mut):
    """per member: how many (path, row) of the fp64 restatement — mutated by `mut` — lie outside the golden bars"""
    n_steps, every = bt.GOLDEN_SHAPE
    case = bt.path_case(rec["model"], n_steps)
    out = [0, 0]
    with mp.workdps(qc.DPS):
        for i in range(bt.GOLDEN_N):
            N = bt.mutated_counts(case, n_steps, d["UJ"][i], mut)
            d64 = bt._float_draws(d, i)
            for m in range(2):
                xs, vT = bt.walk(case, n_steps, float, d64, i, N, m == 1, rec["martingale"], None, mut)
                got = qc.rows_of(case, xs, float, every, 0) + [vT]
                for row in range(6):
                    if abs(mp.mpf(got[row].v) - mp.mpf(rec["want"][m][i][row])) > rec["bars"][m][i][row]:
                        out[m] += 1
    return out


def test_mutations_move_the_restatement_beyond_the_bars(golden_draws):
    """The golden rows are those of the device's path test (the same walk, seeds and bars).  Unmutated, the fp64
    restatement is inside every bar.  Each of the six mutations moves (trajectory, row) pairs outside their bars; a mirror
    that keeps +z moves the mirrors only; none moves var_T, which no jump reaches."""
    recs = {(r["model"], r["martingale"]): r for r in DOC["rows"]}
    assert set(recs) == {(m, k) for m in bt.MODELS for k in (0, 1)}
    for key, rec in recs.items():
        assert misses(rec, golden_draws, None) == [0, 0], key
        found = {mut: misses(rec, golden_draws, mut) for mut in bt.MUTATIONS}
        print(f"\n{key}: (path, row) pairs outside the bars, [trajectories, mirrors], of {6 * bt.GOLDEN_N} each: {found}")
        for mut in ("r_plain", "r_plus", "odd_words", "late_jump", "mean_T"):
            assert min(found[mut]) > 0, (key, mut, found)
        assert found["keep_z"][0] == 0 and found["keep_z"][1] > 0, (key, found)


# ---- the Carr–Madan rule ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(bt.CM_CASES))
def test_carr_madan_rule_against_the_exact_integral(key):
    """hh_fourier.hip's rule for ϕ_B restated in numpy complex128 on the kernel's own panels, against the exactly
    integrated truncated integral of the fixture: inside merton_cases.cm_bar(S0, e64).  A Feller-violating model, a put
    (by parity on the truncated call), λ = 0 (then the Heston golden value's own rule), σ_J = 0, a short expiry."""
    from oracle import carr_madan_fp64 as fp
    case, rec = bt.cm_cases()[key], DOC["carr_madan"][key]
    with mp.workdps(qc.DPS):
        exact = mp.mpf(rec["call"])
        rule = cl.cm_rule_fp64(case, fp.PANELS * fp.subpanels(case["alpha"], case["bound"]), bt.phi)
        miss, bar = float(abs(mp.mpf(rule) - exact)), bt.cm_bar(case["S0"], rec["e64"])
        print(f"\n{key}: rule {rule!r}, |rule − exact| = {miss:.3g}, bar {bar:.3g}")
        assert miss <= bar
        if case["cp"] < 0:
            put = rule + (-case["S0"] + case["K"] * case["discount"])
            assert abs(mp.mpf(put) - (exact + cl.cm_parity(case))) <= bar and put > 0
    if case["lam"] == 0.0:  # no jumps: the rule is the Heston rule's, and the compensator is an exact zero
        other = cl.cm_rule_fp64(dict(case, mu_j=0.3, sigma_j=0.4), fp.PANELS, bt.phi)
        assert other == cl.cm_rule_fp64(case, fp.PANELS, bt.phi)


# ---- routing ---------------------------------------------------------------------------------------------------------------

def bates_inputs(**kw):
    c = dict(bt.LAW, **kw)
    return hh.BatesInputs(REF, c["r_drift"], c["S0"], c["V0"], c["kappa"], c["theta"], c["sigma"], c["rho"], c["lam"],
                          c["mu_j"], c["sigma_j"])


def vanilla(K=100.0, style=None):
    return hh.VanillaOption(K, EXP, style or hh.European(), hh.Call(), hh.Spot())


def _mc(dyn, strat, steps=4, n=8, **kw):
    return hh.MonteCarlo(dyn, strat, hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64)), **kw)


def test_inputs_and_structs():
    bi = bates_inputs()
    assert not isinstance(bi, (hh.HestonInputs, hh.MertonInputs)) and isinstance(hh.BatesDynamics(), hmc.PriceDynamics)
    assert not isinstance(hh.BatesDynamics(), (hh.HestonDynamics, hh.MertonDynamics))
    assert (bi.kappa, bi.theta, bi.sigma, bi.rho) == (0.3, 0.04, 0.9, -0.5) and isinstance(bi.heston(), hh.HestonInputs)
    assert "BatesDynamics" in hh.solve.__doc__ and "BatesInputs" in hh.solve.__doc__
    curve = hh.RateCurve(REF, [0.5, 6.0], zeros=[0.01, 0.04])
    mkt = hh.BatesInputs(REF, curve, 100.0, 0.04, 0.3, 0.04, 0.9, -0.5, 0.8, -0.1, 0.15)
    model, c, (q, j) = routes.BATES.form_structs(vanilla(), mkt, _mc(hh.BatesDynamics(), hh.HestonQE(1.25, True), steps=12))
    assert (c.dynamics, c.strategy, c.n_steps, c.n_partials, c.antithetic) == (_ffi.HH_HESTON, _ffi.HH_QE, 12, 0, 0)
    assert model.r_drift == hh.zero_rate(curve, 0.0) and model.T == hh.yearfrac(REF, EXP) and model.discount == hh.df(curve, EXP)
    assert (model.V0, model.kappa, model.theta, model.sigma, model.rho) == (0.04, 0.3, 0.04, 0.9, -0.5)
    assert (q.psi_c, q.martingale, q.reserved) == (1.25, 1, 0)
    assert (j.lambda_, j.mu_j, j.sigma_j) == (0.8, -0.1, 0.15)


def test_method_errors_name_the_route():
    bi, hi = bates_inputs(), hh.HestonInputs(REF, 0.0, 100.0, 0.04, 0.3, 0.04, 0.9, -0.5)
    mi = hh.MertonInputs(REF, 0.03, 100.0, 0.2, 0.8, -0.1, 0.15)
    good = _mc(hh.BatesDynamics(), hh.HestonQE())
    route = "MonteCarlo(BatesDynamics(), HestonQE(psi_c, martingale), config)"
    refused = [
        (vanilla(), bi, _mc(hh.BatesDynamics(), hh.EulerMaruyama()), route),
        (vanilla(), bi, _mc(hh.BatesDynamics(), hh.HestonBroadieKaya()), route),
        (vanilla(), bi, _mc(hh.BatesDynamics(), hh.MertonExact()), route),
        (vanilla(), bi, _mc(hh.HestonDynamics(), hh.HestonQE()), route),
        (vanilla(), bi, _mc(hh.MertonDynamics(), hh.EulerMaruyama()), route),
        (vanilla(), bi, _mc(hh.LognormalDynamics(), hh.BlackScholesExact()), route),
        (vanilla(), hi, good, route),
        (vanilla(), mi, good, route),
        (vanilla(), bi, hh.CarrMadan(1.0, 32.0, hh.HestonDynamics()), "CarrMadan(alpha, bound, BatesDynamics())"),
        (vanilla(), bi, hh.CarrMadan(1.0, 32.0, hh.MertonDynamics()), "CarrMadan(alpha, bound, BatesDynamics())"),
        (vanilla(), hi, hh.CarrMadan(1.0, 32.0, hh.BatesDynamics()), "on BatesInputs"),
        (vanilla(), bi, _mc(hh.BatesDynamics(), hh.HestonQE(), devices=(0,)), "one device"),
        (vanilla(style=hh.American()), bi, good, "American exercise is not offered on Bates paths"),
        (hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.ContinuousMonitoring()), bi, good,
         "Monitoring"),
        (hh.LookbackOption(EXP, hh.Call(), monitoring=hh.ContinuousMonitoring()), bi, good, "Monitoring"),
        (vanilla(), bates_inputs(S0=hh.Dual(100.0, (1.0,))), good, "FiniteDifference"),
        (vanilla(), bates_inputs(lam=hh.Dual(0.8, (1.0,))), good, "FiniteDifference"),
        (vanilla(), bates_inputs(S0=hh.Dual(100.0, (1.0,))), hh.CarrMadan(1.0, 32.0, hh.BatesDynamics()), "FiniteDifference"),
        (vanilla(), bi, hh.BlackScholesAnalytic(), route),
        (vanilla(style=hh.American()), bi, hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(8, steps=4), 2), route),
    ]
    for payoff, mkt, method, text in refused:
        with pytest.raises(hh.MethodError, match=re.escape(text)):
            hh.solve(hh.PricingProblem(payoff, mkt), method)
    with pytest.raises(hh.MethodError, match="replay"):
        hh.solve(hh.PricingProblem(vanilla(), bi), good, replay=np.zeros(8))
    with pytest.raises(hh.MethodError, match="FiniteDifference"):  # ForwardAD: no partials are carried
        hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla(), bi), hh.SpotLens()), hh.ForwardAD(), good)
    with pytest.raises(hh.MethodError, match=re.escape(route)):
        hh.solve(hh.BasketPricingProblem([vanilla(), vanilla(90.0)], bi), _mc(hh.BatesDynamics(), hh.EulerMaruyama()))
    assert hmc.solve_montecarlo_many([hh.PricingProblem(vanilla(), bi)] * 2, good) is None  # plain solves, one by one


def test_basket_groups_share_one_simulation(monkeypatch):
    from hedgehog_jl_amd import basket as hb
    bi = bates_inputs()
    later = hh.Date(2027, 1, 1)
    payoffs = [hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2)), vanilla(95.0),
               hh.DigitalOption(101.0, EXP, hh.Put()), hh.VanillaOption(110.0, later, hh.European(), hh.Put(), hh.Spot()),
               hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(2))]
    calls = []

    def fake_paths(group, market_inputs, method, ensemble=True, route=None):
        calls.append([payoffs.index(p) if p in payoffs else p.strike for p in group])
        return [hh.MonteCarloSolution(hh.PricingProblem(p, market_inputs), method, 0.0) for p in group]

    monkeypatch.setattr(hb, "solve_path_payoffs", fake_paths)
    sol = hh.solve(hh.BasketPricingProblem(payoffs, bi), _mc(hh.BatesDynamics(), hh.HestonQE()))
    assert calls == [[0, 1, 2, 4], [3]] and all(s is not None for s in sol.solutions)
    calls.clear()
    hh.solve(hh.BasketPricingProblem([vanilla(96.0), vanilla(106.0)], bi), _mc(hh.BatesDynamics(), hh.HestonQE()))
    assert calls == [[96.0, 106.0]]  # European vanillas alone: the vanilla kind, monitored at expiry
