"""Merton jump diffusion on the host side, without a GPU: the struct and the three entry points declared, exported and
bound; the closed forms held against each other at 50 digits; the Poisson inversion of csrc/hh_jump.h, as a stand-alone
host program (also under AddressSanitizer and UBSan), against the exact restatement; the fixture's own conditions and
its maker; how the new Python types are routed, grouped and refused."""
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
from hedgehog_jl_amd import montecarlo as hmc  # noqa: E402
from hedgehog_jl_amd import routes  # noqa: E402
from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import merton_cases as mc  # noqa: E402
from tests import oracle_ffi  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_solve_jump": 6, "hh_mc_solve_path_jump": 11, "hh_carr_madan_jump": 12}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
DOC = mc.load_golden()


def merton_inputs(**kw):
    c = dict(mc.BASE, **kw)
    return hh.MertonInputs(REF, c["r_drift"], c["S0"], c["sigma"], c["lam"], c["mu_j"], c["sigma_j"])


def vanilla(K=105.0, side=None):
    return hh.VanillaOption(K, EXP, hh.European(), side or hh.Call(), hh.Spot())


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_hh_jump_layout(tmp_path):
    """hh_jump is 24 bytes, three doubles at 0, 8 and 16: a compiled offsetof dump against the ctypes structure"""
    fields = ["lambda", "mu_j", "sigma_j"]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(hh_jump));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(hh_jump, {f}), sizeof(((hh_jump*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, env=host_env()).stdout.split("\n")
    assert out[0] == "sizeof 24" and C.sizeof(_ffi.hh_jump) == 24
    got = [(n.rstrip("_"), getattr(_ffi.hh_jump, n).offset, getattr(_ffi.hh_jump, n).size) for n, _ in _ffi.hh_jump._fields_]
    want = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:4]]
    assert got == want == [("lambda", 0, 8), ("mu_j", 8, 8), ("sigma_j", 16, 8)]
    j = _ffi.make_jump(0.8, -0.1, 0.15)
    assert (j.lambda_, j.mu_j, j.sigma_j) == (0.8, -0.1, 0.15)


def test_new_prototypes_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bound = {s[0]: s for s in _ffi.SYMBOLS}
    lib = _ffi.load_library()
    assert open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hedgehog_mc.map")).read().count("global: hh_*;") == 1
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines()}
    for name, arity in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == arity, name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == arity, name
        assert getattr(lib, name) is not None and name in exported
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    assert re.search(r"#define HH_JUMP_MAX_MEAN\s+64\.0\b", hdr) and _ffi.HH_JUMP_MAX_MEAN == 64.0
    assert re.search(r"#define HH_JUMP_MAX_COUNT\s+255\b", hdr) and _ffi.HH_JUMP_MAX_COUNT == 255
    assert "hh_jump.hip" in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "kDomJump = 4u" in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_rng.h")).read() and mc.DOM_JUMP == 4


# ---- the closed forms at 50 digits -------------------------------------------------------------------------------------

@pytest.mark.parametrize("bound", [300.0, 400.0])
def test_series_equals_the_exactly_integrated_carr_madan_integral(bound):
    """σ²T·bound²/2 > 1000: the integrand beyond ±bound is below e⁻¹⁰⁰⁰, so the truncated integral IS the price, and
    Merton's series is the same number — two formulas that share nothing but the model."""
    assert mc.BASE["sigma"] ** 2 * mc.BASE["T"] * bound ** 2 / 2 > 1000
    for K in (105.0, 80.0):  # (puts are calls by parity in both formulas: test_parity_and_the_limit_without_jumps)
        case = cl.cm_case(mc.BASE, K, 1.0, bound)
        with mp.workdps(mc.DPS):
            # (the case carries its discount factor, a double: the series takes the same one)
            assert abs(cl.cm_exact_call(case, mc.log_cf) - mc.series(case, K, 1.0)) < mp.mpf(10) ** -30, K
    assert mp.nstr(mc.series(mc.BASE, 105.0, 1.0), 18) == "8.97843684569237133"
    assert DOC["series"]["price"] == mp.nstr(mc.series(mc.BASE, 105.0, 1.0), 30)


def test_parity_and_the_limit_without_jumps():
    with mp.workdps(mc.DPS):
        for K in (70.0, 100.0, 140.0):
            call, put = mc.series(mc.BASE, K, 1.0), mc.series(mc.BASE, K, -1.0)
            D = mp.exp(-mp.mpf(mc.BASE["r_drift"]) * mp.mpf(mc.BASE["T"]))
            assert abs(call - put - (mp.mpf(mc.BASE["S0"]) - mp.mpf(K) * D)) < mp.mpf(10) ** -40
            flat = dict(mc.BASE, lam=0.0)
            for cp in (1.0, -1.0):
                assert abs(mc.series(flat, K, cp) - mc.black_scholes(flat, K, cp)) < mp.mpf(10) ** -40
            # jumps of size zero are no jumps, whatever their intensity
            assert abs(mc.series(dict(mc.BASE, mu_j=0.0, sigma_j=0.0), K, 1.0) - mc.black_scholes(flat, K, 1.0)) < mp.mpf(10) ** -40
        # the digitals of the law tests: a call and a put digital pay `cash` between them
        both = mc.series(mc.BASE, 102.0, 1.0, digital_cash=3.0) + mc.series(mc.BASE, 102.0, -1.0, digital_cash=3.0)
        assert abs(both - 3 * mp.exp(-mp.mpf(mc.BASE["r_drift"]))) < mp.mpf(10) ** -40


def test_the_host_series_is_the_50_digit_series():
    for K, side, cp in ((105.0, hh.Call(), 1.0), (90.0, hh.Put(), -1.0)):
        got = hh.solve(hh.PricingProblem(vanilla(K, side), merton_inputs()), hh.MertonAnalytic()).price
        T = hh.yearfrac(REF, EXP)
        want = mc.series(dict(mc.BASE, T=T), K, cp)
        assert abs(got - float(want)) <= 1e-13 * mc.BASE["S0"]
    assert hh.merton_series(100.0, 105.0, 1.0, 0.2, 0.8, -0.1, 0.15, 1.0, math.exp(-0.03)) == pytest.approx(8.978436845692371, abs=1e-13)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(vanilla(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)), hh.MertonAnalytic())


# ---- the Poisson inversion ---------------------------------------------------------------------------------------------

def test_fixture_uniforms_keep_their_margin():
    """every fixture U lies at least 1e-9 from every exact cumulative boundary: fp64 rounding of the sum, about 1e-16,
    cannot move N — and the Python-float restatement of the loop agrees with the exact inversion on every one"""
    assert DOC["margin"] == mc.MARGIN == 1e-9
    means = []
    for rec in DOC["poisson"]:
        m = float.fromhex(rec["m"])
        means.append(m)
        for u, n in zip(rec["U"], rec["N"]):
            u = float.fromhex(u)
            exact, dist = mc.poisson_exact(u, m)
            assert exact == n == mc.poisson_fp64(u, m) and (dist >= mc.MARGIN or m == 0.0), (u, m)
            assert u == mc.uniform_of(int(u * 2.0 ** 52))  # a uniform the device can draw
        assert m == 0.0 or len(set(rec["N"])) >= 3, m
        assert m > 0.0 or set(rec["N"]) == {0}
    assert means == [0.0, 1e-3, 1.0, 8.0, 64.0]


def _build_host_check(tmp_path, flags, name):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "jump_host_check.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_poisson_inversion_host_program(tmp_path, build):
    """tests/c/jump_host_check.cpp — its own main, csrc/hh_jump.h included — returns the exact inversion's N on every
    fixture pair, and ends with N <= 255 at U = 2⁻⁵³ and U = 1 − 2⁻⁵³, where the cap or saturation decides.  Built
    plainly and with -fsanitize=address,undefined, and run as a program: nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = _build_host_check(tmp_path, flags, "jump_host_check_" + build)
    pairs, want = [], []
    for rec in DOC["poisson"]:
        pairs += [(u, rec["m"]) for u in rec["U"]]
        want += rec["N"]
    n_regular = len(pairs)
    pairs += [(e["U"], e["m"]) for e in DOC["edges"]]
    (tmp_path / "pairs.txt").write_text("".join(f"{u} {m}\n" for u, m in pairs))
    run = subprocess.run([exe, str(tmp_path / "pairs.txt")], capture_output=True, text=True, env=host_env(), timeout=60)
    assert run.returncode == 0, run.stderr
    got = [int(t) for t in run.stdout.split()]
    assert len(got) == len(pairs) and got[:n_regular] == want
    edges = got[n_regular:]
    assert all(0 <= n <= mc.MAX_COUNT for n in edges)
    assert edges == [e["N"] for e in DOC["edges"]]  # the fp64 loop, operation for operation
    assert {(float.fromhex(e["U"]), float.fromhex(e["m"])) for e in DOC["edges"]} >= \
        {(u, m) for m in (0.0, 1e-3, 1.0, 8.0, 64.0) for u in (2.0 ** -53, 1.0 - 2.0 ** -53)}
    by = {(float.fromhex(e["U"]), float.fromhex(e["m"])): n for e, n in zip(DOC["edges"], edges)}
    assert by[(1.0 - 2.0 ** -53, 2.5)] == mc.MAX_COUNT  # the sum saturates at 1 − 2⁻⁵²: the cap is what ends the search
    assert by[(2.0 ** -53, 0.0)] == by[(1.0 - 2.0 ** -53, 0.0)] == 0 and by[(2.0 ** -53, 64.0)] > 0


def test_maker_regenerates_the_fixture_identically():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_merton_exact", os.path.join(ROOT, "tests", "golden", "make_merton_exact.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    again = json.loads(json.dumps(maker.build(oracle_ffi.load())))
    assert again == DOC
    shapes = {b["id"]: len(b["payoffs"]) for b in DOC["carr_madan"]}
    assert shapes == {"single": 1, "basket33": 33, "lambda0": 3}
    for r in DOC["counts"]["path"]:  # λ·dt near 1: N takes 0 … 4 within one case
        N = np.array(r["N"])
        assert N.shape == (mc.PATH_N, r["n_steps"]) and all((N == k).any() for k in range(5))


def test_restatement_without_jumps_is_the_lognormal_scheme():
    """tests/merton_cases.py's walk at λ = 0 is oracle/euler_exact.py's lognormal path, value for value"""
    from oracle import euler_exact as ex
    case = dict(mc.path_case(5, 0), lam=0.0, V0=0.0, kappa=0.0, theta=0.0, discount=1.0, dynamics="lognormal", em_split=1)
    dW = [0.1, -0.2, 0.05, 0.3, -0.15]
    with mp.workdps(mc.DPS):
        rows = mc.path_member(case, mp.mpf, dW, [0] * 5, [None] * 5, False, 1, False)
        ref = ex.run(dict(case, dW=[[[t] for t in dW]]), mp.mpf, [(100.0, 1.0)])[0]
        assert rows[4].v == ref["S"][0][0]


# ---- routing ---------------------------------------------------------------------------------------------------------------

def _mc(dyn, strat, steps=4, n=8, **kw):
    return hh.MonteCarlo(dyn, strat, hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64)), **kw)


def test_method_errors():
    """every (dynamics, strategy, inputs) mix outside the Merton routes is a MethodError, before any device is touched"""
    mi, bs = merton_inputs(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    asian = hh.AsianOption(100.0, EXP, hh.Call())
    cont = hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.ContinuousMonitoring())
    refused = [
        (vanilla(), mi, _mc(hh.LognormalDynamics(), hh.EulerMaruyama())),
        (vanilla(), mi, _mc(hh.LognormalDynamics(), hh.BlackScholesExact())),
        (vanilla(), mi, _mc(hh.HestonDynamics(), hh.HestonBroadieKaya())),
        (vanilla(), mi, _mc(hh.MertonDynamics(), hh.BlackScholesExact())),
        (vanilla(), bs, _mc(hh.MertonDynamics(), hh.EulerMaruyama())),
        (vanilla(), bs, _mc(hh.MertonDynamics(), hh.MertonExact())),
        (vanilla(), bs, _mc(hh.LognormalDynamics(), hh.MertonExact())),
        (asian, mi, _mc(hh.MertonDynamics(), hh.MertonExact())),                # the terminal law has no path
        (cont, mi, _mc(hh.MertonDynamics(), hh.EulerMaruyama())),               # no bridge across a jump
        (vanilla(), mi, _mc(hh.MertonDynamics(), hh.MertonExact(), devices=(0,))),
        (hh.VanillaOption(105.0, EXP, hh.American(), hh.Call(), hh.Spot()), mi, _mc(hh.MertonDynamics(), hh.EulerMaruyama())),
        (vanilla(), hh.MertonInputs(REF, 0.03, hh.Dual(100.0, (1.0,)), 0.2, 0.8, -0.1, 0.15), _mc(hh.MertonDynamics(), hh.MertonExact())),
        (vanilla(), hh.MertonInputs(REF, 0.03, 100.0, 0.2, hh.Dual(0.8, (1.0,)), -0.1, 0.15), _mc(hh.MertonDynamics(), hh.EulerMaruyama())),
    ]
    for payoff, mkt, method in refused:
        with pytest.raises(hh.MethodError):
            hh.solve(hh.PricingProblem(payoff, mkt), method)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(vanilla(), mi), _mc(hh.MertonDynamics(), hh.MertonExact()), replay=np.zeros(8))
    for method in (hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics()), hh.CarrMadan(1.0, 32.0, hh.HestonDynamics())):
        with pytest.raises(hh.MethodError):
            hh.solve(hh.PricingProblem(vanilla(), mi), method)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(vanilla(), bs), hh.CarrMadan(1.0, 32.0, hh.MertonDynamics()))
    with pytest.raises(hh.MethodError):  # ForwardAD: no partials are carried
        hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla(), mi), hh.SpotLens()), hh.ForwardAD(),
                 _mc(hh.MertonDynamics(), hh.MertonExact()))
    with pytest.raises(hh.MethodError):
        hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla(), mi), hh.optic("market_inputs.jump_intensity")), hh.ForwardAD(),
                 hh.CarrMadan(1.0, 32.0, hh.MertonDynamics()))
    # several Merton problems never share an hh_mc_solve_multi pass
    assert hmc.solve_montecarlo_many([hh.PricingProblem(vanilla(), mi)] * 2, _mc(hh.MertonDynamics(), hh.MertonExact())) is None


def test_structs_of_a_merton_solve():
    """MertonExact: the exact law's dates (r_drift = zero_rate(rate, expiry)) and the correct ·T drift; EulerMaruyama:
    r_drift = zero_rate(rate, 0.0) as every Euler solve; the jump fields travel in hh_jump"""
    curve = hh.RateCurve(REF, [0.5, 2.0], zeros=[0.01, 0.04])
    mi = hh.MertonInputs(REF, curve, 100.0, 0.2, 0.8, -0.1, 0.15)
    prob = hh.PricingProblem(vanilla(), mi)
    model, c, (jump,) = routes.MERTON_LAW.form_structs(prob.payoff, mi, _mc(hh.MertonDynamics(), hh.MertonExact(), compat_sqrt_alpha=True))
    assert (c.dynamics, c.strategy, c.compat_sqrt_alpha, c.n_partials) == (mc.GBM, mc.EXACT, 0, 0)
    assert model.r_drift == hh.zero_rate(curve, EXP) and model.T == hh.yearfrac(REF, EXP) and model.sigma == 0.2
    assert (jump.lambda_, jump.mu_j, jump.sigma_j) == (0.8, -0.1, 0.15)
    model, c, (jump,) = routes.MERTON.form_structs(prob.payoff, mi, _mc(hh.MertonDynamics(), hh.EulerMaruyama(), steps=12))
    assert (c.dynamics, c.strategy, c.n_steps) == (mc.GBM, mc.EULER, 12) and model.r_drift == hh.zero_rate(curve, 0.0)
    assert model.discount == hh.df(curve, EXP)


def test_basket_grouping(monkeypatch):
    """Euler groups share one simulation through the existing grouping — the vanillas of an expiry ride along, or form a
    path group of their own where there is none; MertonExact baskets loop over solves"""
    from hedgehog_jl_amd import basket as hb
    mi = merton_inputs()
    later = hh.Date(2023, 1, 1)
    payoffs = [hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2)), vanilla(95.0),
               hh.DigitalOption(101.0, EXP, hh.Put()), hh.VanillaOption(110.0, later, hh.European(), hh.Put(), hh.Spot()),
               hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(2))]
    calls = []

    def fake_paths(group, market_inputs, method, ensemble=True, route=None):
        calls.append(("path", [payoffs.index(p) for p in group]))
        assert market_inputs is mi
        return [hh.MonteCarloSolution(hh.PricingProblem(p, market_inputs), method, 0.0) for p in group]

    def fake_solve(prob, method, ensemble=True):
        calls.append(("solve", prob.payoff.strike))
        return hh.MonteCarloSolution(prob, method, 0.0)

    monkeypatch.setattr(hb, "solve_path_payoffs", fake_paths)
    monkeypatch.setattr(hb, "solve_montecarlo", fake_solve)
    sol = hh.solve(hh.BasketPricingProblem(payoffs, mi), _mc(hh.MertonDynamics(), hh.EulerMaruyama()))
    assert calls == [("path", [0, 1, 2, 4]), ("path", [3])] and all(s is not None for s in sol.solutions)
    calls.clear()
    vanillas = [vanilla(95.0), vanilla(105.0, hh.Put())]
    hh.solve(hh.BasketPricingProblem(vanillas, mi), _mc(hh.MertonDynamics(), hh.MertonExact()))
    assert calls == [("solve", 95.0), ("solve", 105.0)]


def test_fd_lenses_set_the_jump_fields():
    """the lens machinery is generic: SpotLens, VolLens and an optic on a jump field bump a MertonInputs in place of a copy"""
    prob = hh.PricingProblem(vanilla(), merton_inputs())
    up = hh.set(prob, hh.optic("market_inputs.jump_intensity"), 0.9)
    assert up.market_inputs.jump_intensity == 0.9 and prob.market_inputs.jump_intensity == 0.8
    assert hh.optic("market_inputs.jump_mean")(prob) == -0.1 and hh.optic("market_inputs.jump_std")(prob) == 0.15
    assert hh.set(prob, hh.SpotLens(), 101.0).market_inputs.spot == 101.0
    vol = hh.VolLens(105.0, EXP)
    assert vol(prob) == 0.2 and hh.set(prob, vol, 0.25).market_inputs.sigma.σ == 0.25
    assert isinstance(hh.set(prob, vol, 0.25).market_inputs, hh.MertonInputs)
    # a central difference through the host series: ∂price/∂λ > 0 for a call (jumps add variance)
    g = hh.solve(hh.GreekProblem(prob, hh.optic("market_inputs.jump_intensity")), hh.FiniteDifference(1e-4), hh.MertonAnalytic())
    h = 1e-4 * 0.8
    want = (mc.series(dict(mc.BASE, T=hh.yearfrac(REF, EXP), lam=0.8 + h), 105.0, 1.0) -
            mc.series(dict(mc.BASE, T=hh.yearfrac(REF, EXP), lam=0.8 - h), 105.0, 1.0)) / (2 * h)
    assert g.greek > 0 and g.greek == pytest.approx(float(want), rel=1e-8)
