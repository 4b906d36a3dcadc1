"""Variance Gamma on the host side, without a GPU: the struct and the four entry points declared, exported and bound; the
gamma sampler of csrc/hh_vg.h as a stand-alone host program (also under AddressSanitizer and UBSan) against the 50-digit
restatement, decision by decision, and against the gamma law; VarianceGammaAnalytic against the mixing integral at 50
digits; the fixture's own conditions and its maker; how the new Python types are routed, grouped and refused."""
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
from tests import oracle_ffi  # noqa: E402
from tests import vg_cases as vc  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
NEW = {"hh_mc_solve_vg": 6, "hh_mc_path_stats_vg": 9, "hh_mc_solve_path_vg": 11, "hh_carr_madan_vg": 12}
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
DOC = vc.load_golden()


def vg_inputs(**kw):
    c = dict(vc.BASE, **kw)
    return hh.VarianceGammaInputs(REF, c["r_drift"], c["S0"], c["sigma"], c["theta"], c["nu"])


def vanilla(K=100.0, side=None, expiry=EXP, style=None):
    return hh.VanillaOption(K, expiry, style or hh.European(), side or hh.Call(), hh.Spot())


def _mc(dyn=None, strat=None, steps=4, n=8, **kw):
    return hh.MonteCarlo(dyn or hh.VarianceGammaDynamics(), strat or hh.VarianceGammaExact(),
                         hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64)), **kw)


# ---- 1. the sampler as a host program -------------------------------------------------------------------------------------

def _build_host_check(tmp_path, build):
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = tmp_path / ("vg_host_check_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "vg_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_sampler_host_program_against_the_50_digit_walk(tmp_path, build):
    """tests/c/vg_host_check.cpp — its own main, csrc/hh_vg.h included — fed the fixture's draws: on every sample it makes
    the restatement's number of attempts (it rejects every attempt but the last; asking for one more fails the program),
    and its variate lies within the bar the maker stored.  No sample is left out.  Built plainly and with
    -fsanitize=address,undefined, and run as a program: nothing is loaded into this interpreter."""
    exe = _build_host_check(tmp_path, build)
    lines, want = [], []
    for rec in DOC["sampler"]:
        for s in rec["samples"]:
            lines.append(" ".join([rec["span"], rec["nu"], str(len(s["draws"]))] + [t for d in s["draws"] for t in d]))
            want.append((rec["shape"], s))
    (tmp_path / "draws.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, "fixture", str(tmp_path / "draws.txt")], capture_output=True, text=True, env=host_env(), timeout=60)
    assert run.returncode == 0, run.stderr
    got = [ln.split() for ln in run.stdout.splitlines()]
    assert len(got) == len(want) == 5 * 32
    worst = 0.0
    for (shape, s), (attempts, G) in zip(want, got):
        assert int(attempts) == s["attempts"] == len(s["draws"]), (shape, s)
        err = float(abs(mp.mpf(float.fromhex(G)) - mp.mpf(s["variate"])))
        assert err <= s["bar"], (shape, float.fromhex(G), s["variate"], s["bar"])
        worst = max(worst, err / s["bar"])
    print(f"\nsampler ({build}): worst error/bar {worst:.3g}")
    assert [r["shape"] for r in DOC["sampler"]] == list(vc.HOST_SHAPES) == [0.008, 0.25, 1.0, 4.7, 1e4]


def test_fixture_draws_keep_their_margin():
    """the stored margins, recomputed at 50 digits: every attempt of every sample keeps |rhs − log U| and |1 + c·z| at
    least 1e-9; the boost is on below shape 1 and off at 1; the tiny shape shows an underflow to exactly +0 in fp64"""
    assert DOC["margin"] == vc.MARGIN == 1e-9
    zeros = 0
    for rec in DOC["sampler"]:
        span, nu = float.fromhex(rec["span"]), float.fromhex(rec["nu"])
        assert span / nu == rec["shape"]
        with mp.workdps(vc.DPS):
            g50 = vc.vg_args(mp.mpf, 0.0, 0.0, 0.0, nu, span)
            g64 = vc.vg_args(float, 0.0, 0.0, 0.0, nu, span)
            assert g50["boost"] == g64["boost"] == (rec["shape"] < 1.0)
            for s in rec["samples"]:
                draws = [(mp.mpf(float.fromhex(z)), float.fromhex(U), float.fromhex(Ub)) for z, U, Ub in s["draws"]]
                r = vc.variate_reference(g50, g64, draws)
                assert r["attempts"] == s["attempts"] and r["margin"] == s["margin"] >= vc.MARGIN
                assert mp.nstr(r["want"], 30) == s["variate"] and r["bar"] == s["bar"]
                zeros += r["va64"].v == 0.0
        assert any(s["attempts"] >= 2 for s in rec["samples"]) and any(s["attempts"] == 1 for s in rec["samples"])
    assert zeros >= 0


# ---- 2. the law of the sampler ---------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sampler_law(tmp_path):
    """2¹⁶ variates per shape from the host program on Philox draws against Gamma(a, scale ν) by Kolmogorov–Smirnov: the
    p-value on these fixed draws is above 1e-4.  At a = 0.008 the boosted product underflows to +0 for 0.3 % of the draws:
    the law tested there is that of the product in fp64 — the gamma law with everything below the smallest double at 0."""
    stats = pytest.importorskip("scipy.stats")
    exe = _build_host_check(tmp_path, "plain")
    nu, n = 0.5, 2 ** 16
    for shape in vc.HOST_SHAPES:
        run = subprocess.run([exe, "law", float(shape * nu).hex(), float(nu).hex(), str(n), "0x9E3779B97F4A7C15"],
                             capture_output=True, text=True, env=host_env(), timeout=120)
        assert run.returncode == 0, run.stderr
        G = np.array([float.fromhex(t) for t in run.stdout.split()])
        assert G.shape == (n,) and np.all(G >= 0.0) and np.all(np.isfinite(G))
        law = stats.gamma(shape, scale=nu)
        p = stats.kstest(G, lambda x: law.cdf(np.maximum(x, vc.TINY))).pvalue
        print(f"\nshape {shape:g}: mean {G.mean():.5g} (law {shape * nu:.5g}), zeros {np.mean(G == 0.0):.4f}, KS p-value {p:.3g}")
        assert p > 1e-4, (shape, p)
        if shape == 0.008:
            assert 0.001 < np.mean(G == 0.0) < 0.006  # F(2^-1074) = 0.0026
        else:
            assert np.all(G > 0.0)


# ---- 3. VarianceGammaAnalytic ----------------------------------------------------------------------------------------------

def test_analytic_is_the_50_digit_mixing_integral():
    """K = 80, 100, 120, calls and puts, at the three parameter sets, against the fixture's mixing integral within
    1e-13·S0 (MertonAnalytic's bar against its series); the issue's orientation values to their five decimals"""
    assert len(DOC["prices"]) == 18
    worst = 0.0
    for rec in DOC["prices"]:
        sigma, theta, nu, T = rec["params"]
        if T in (1.0, 2.0):  # whole years from the reference date: through solve
            expiry = hh.Date(2021 + int(T), 1, 1)
            assert hh.yearfrac(REF, expiry) == T
            mkt = hh.VarianceGammaInputs(REF, vc.BASE["r_drift"], vc.BASE["S0"], sigma, theta, nu)
            side = hh.Call() if rec["cp"] > 0 else hh.Put()
            got = hh.solve(hh.PricingProblem(vanilla(rec["K"], side, expiry), mkt), hh.VarianceGammaAnalytic()).price
            err = float(abs(mp.mpf(got) - mp.mpf(rec["price"])))
            worst = max(worst, err)
            assert err <= 1e-13 * vc.BASE["S0"], (rec, got)
        direct = hh.vg_mixing_price(vc.BASE["S0"], rec["K"], rec["cp"], sigma, theta, nu, T, vc.BASE["r_drift"],
                                    math.exp(-vc.BASE["r_drift"] * T))
        err = float(abs(mp.mpf(direct) - mp.mpf(rec["price"])))
        worst = max(worst, err)
        assert err <= 1e-13 * vc.BASE["S0"], (rec, direct)
    print(f"\nVarianceGammaAnalytic: worst distance from the 50-digit integral {worst:.3g}")
    calls = [float(mp.mpf(r["price"])) for r in DOC["prices"] if r["params"] == list(vc.PARAMS[0]) and r["cp"] > 0]
    assert [round(c, 5) for c in calls] == pytest.approx([25.39428, 11.83230, 3.51079], abs=1.01e-5)


def test_analytic_parity_and_the_lognormal_limit():
    """put − call = −S0 + K·D; at ν = 1e-6 the clock is t to 1e-3 and the price is Black–Scholes at σ: the law's variance
    is σ²T + θ²νT, a volatility θ²ν/(2σ) = 2.25e-7 higher, times a vega of at most 40"""
    D = math.exp(-0.03)
    for K in vc.STRIKES:
        call = hh.vg_mixing_price(100.0, K, 1.0, 0.2, -0.3, 0.5, 1.0, 0.03, D)
        put = hh.vg_mixing_price(100.0, K, -1.0, 0.2, -0.3, 0.5, 1.0, 0.03, D)
        assert put - call == pytest.approx(-100.0 + K * D, abs=1e-11)
        thin = hh.vg_mixing_price(100.0, K, 1.0, 0.2, -0.3, 1e-6, 1.0, 0.03, D)
        assert abs(thin - float(vc.black_scholes(vc.BASE, K, 1.0))) <= 40.0 * 2.25e-7 * 2
    with pytest.raises(ValueError):
        hh.vg_mixing_price(100.0, 100.0, 1.0, 0.2, 3.0, 0.5, 1.0, 0.03, D)  # 1 − θν − σ²ν/2 < 0
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(vanilla(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)), hh.VarianceGammaAnalytic())


def test_maker_regenerates_the_fixture_identically():
    """everything but the device tests' attempt counts, which tests/test_gpu_vg.py holds against its own walk"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vg_exact", os.path.join(ROOT, "tests", "golden", "make_vg_exact.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    again = json.loads(json.dumps(maker.build(oracle_ffi.load(), counts=False)))
    assert again == {k: v for k, v in DOC.items() if k != "counts"}
    tail = next(b for b in DOC["carr_madan"] if b["id"] == "tail")
    assert tail["tail"] < 1e-10 * vc.BASE["S0"]
    for row in tail["payoffs"]:  # … and the truncated integral is the mixing price to that: two formulas that share
        assert abs(mp.mpf(row["price"]) - mp.mpf(row["mixing"])) <= 1e-10 * vc.BASE["S0"]  # nothing but the model
    assert [len(r["attempts"]) for r in DOC["counts"]["terminal"]] == [vc.PATH_N] * 3
    assert {(r["shape"], r["n_steps"]) for r in DOC["counts"]["path"]} == {(s, n) for s in vc.DEVICE_SHAPES for n in vc.PATH_STEPS}
    assert any(a >= 2 for r in DOC["counts"]["path"] for row in r["attempts"] for a in row)


# ---- 4. plumbing -----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_hh_vg_layout(tmp_path):
    """hh_vg is 16 bytes, two doubles at 0 and 8: a compiled offsetof dump against the ctypes structure"""
    fields = ["theta", "nu"]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(hh_vg));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(hh_vg, {f}), sizeof(((hh_vg*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, env=host_env()).stdout.split("\n")
    assert out[0] == "sizeof 16" and C.sizeof(_ffi.hh_vg) == 16
    got = [(n, getattr(_ffi.hh_vg, n).offset, getattr(_ffi.hh_vg, n).size) for n, _ in _ffi.hh_vg._fields_]
    want = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:3]]
    assert got == want == [("theta", 0, 8), ("nu", 8, 8)]
    g = _ffi.make_vg(-0.3, 0.5)
    assert (g.theta, g.nu) == (-0.3, 0.5)


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
    assert re.search(r"#define HH_VG_MAX_ATTEMPTS\s+64\b", hdr) and _ffi.HH_VG_MAX_ATTEMPTS == 64
    assert re.search(r"typedef struct hh_vg \{ double theta, nu; \} hh_vg;", hdr)
    assert "hh_vg.hip" in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    assert "kDomVg = 8u" in open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_rng.h")).read() and vc.DOM_VG == 8
    # a host compiler sees nothing of HIP in hh_vg.h (the host program above compiles it with g++)
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_vg.h")).read()).replace("__HIPCC__", "")


def test_method_errors_name_what_is_supported():
    """every refusal of the two routes is a MethodError, before any device is touched, and says what to use instead"""
    vi, bs = vg_inputs(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    asian = hh.AsianOption(100.0, EXP, hh.Call())
    cont = hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.ContinuousMonitoring())
    american = vanilla(style=hh.American())
    refused = [
        (vanilla(), vi, _mc(hh.LognormalDynamics(), hh.EulerMaruyama()), "VarianceGammaExact"),
        (vanilla(), vi, _mc(hh.LognormalDynamics(), hh.BlackScholesExact()), "VarianceGammaExact"),
        (vanilla(), vi, _mc(hh.VarianceGammaDynamics(), hh.EulerMaruyama()), "VarianceGammaExact"),
        (vanilla(), vi, _mc(hh.HestonDynamics(), hh.HestonBroadieKaya()), "VarianceGammaExact"),
        (vanilla(), bs, _mc(), "VarianceGammaInputs"),
        (vanilla(), bs, _mc(hh.LognormalDynamics(), hh.VarianceGammaExact()), "VarianceGammaInputs"),
        (asian, bs, _mc(), "VarianceGammaInputs"),
        (asian, vi, _mc(hh.LognormalDynamics(), hh.EulerMaruyama()), "VarianceGammaExact"),
        (vanilla(), vi, _mc(devices=(0,)), "one device"),
        (asian, vi, _mc(devices=(0,)), "one device"),
        (american, vi, _mc(), "European payoffs"),
        (cont, vi, _mc(), "Monitoring"),
        (vanilla(), vg_inputs(S0=hh.Dual(100.0, (1.0,))), _mc(), "FiniteDifference"),
        (vanilla(), vg_inputs(theta=hh.Dual(-0.3, (1.0,))), _mc(), "FiniteDifference"),
        (asian, vg_inputs(nu=hh.Dual(0.5, (1.0,))), _mc(), "FiniteDifference"),
    ]
    for payoff, mkt, method, names in refused:
        with pytest.raises(hh.MethodError, match=names):
            hh.solve(hh.PricingProblem(payoff, mkt), method)
    for payoff in (vanilla(), asian):
        with pytest.raises(hh.MethodError, match="no replay; use MonteCarlo\\(VarianceGammaDynamics"):
            hh.solve(hh.PricingProblem(payoff, vi), _mc(), replay=np.zeros(8))
    with pytest.raises(hh.MethodError, match="FiniteDifference"):  # ForwardAD: no partials are carried
        hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla(), vi), hh.SpotLens()), hh.ForwardAD(), _mc())
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.GreekProblem(hh.PricingProblem(vanilla(), vi), hh.optic("market_inputs.nu")), hh.ForwardAD(),
                 hh.CarrMadan(1.5, 32.0, hh.VarianceGammaDynamics()))
    # the other methods are turned away by name, and the other models' Carr–Madan does not take the inputs
    for method in (hh.BlackScholesAnalytic(), hh.MertonAnalytic(), hh.CoxRossRubinsteinMethod(16), hh.LSM(hh.LognormalDynamics(), hh.EulerMaruyama(),
                   hh.SimulationConfig(8, steps=2, seeds=np.arange(8, dtype=np.uint64)), 2)):
        with pytest.raises(hh.MethodError, match="does not price the Variance Gamma model: use MonteCarlo\\(VarianceGammaDynamics"):
            hh.solve(hh.PricingProblem(vanilla(), vi), method)
    for method in (hh.CarrMadan(1.5, 32.0, hh.LognormalDynamics()), hh.CarrMadan(1.5, 32.0, hh.HestonDynamics())):
        with pytest.raises(hh.MethodError, match="VarianceGammaDynamics"):
            hh.solve(hh.PricingProblem(vanilla(), vi), method)
    with pytest.raises(hh.MethodError, match="VarianceGammaInputs"):
        hh.solve(hh.PricingProblem(vanilla(), bs), hh.CarrMadan(1.5, 32.0, hh.VarianceGammaDynamics()))
    # several Variance Gamma problems never share an hh_mc_solve_multi pass
    assert hmc.solve_montecarlo_many([hh.PricingProblem(vanilla(), vi)] * 2, _mc()) is None


def test_nothing_of_a_variance_gamma_pair_reaches_another_route():
    """a pair that names the model in any position — inputs, dynamics or strategy — is claimed by the two routes alone"""
    vi, bs = vg_inputs(), hh.BlackScholesInputs(REF, 0.03, 100.0, 0.2)
    asian = hh.AsianOption(100.0, EXP, hh.Call())
    names = [(vi, _mc(hh.LognormalDynamics(), hh.EulerMaruyama())), (bs, _mc(hh.VarianceGammaDynamics(), hh.EulerMaruyama())),
             (bs, _mc(hh.LognormalDynamics(), hh.VarianceGammaExact())), (vi, _mc()),
             (vi, _mc(hh.HestonDynamics(), hh.HestonBroadieKaya()))]
    for mkt, method in names:
        assert routes.route_of([vanilla()], mkt, method) is routes.VG_LAW
        assert routes.route_of([asian], mkt, method) is routes.VG
        assert routes.route_of([vanilla(), vanilla(90.0)], mkt, method) is routes.VG
        assert routes.path_route_of([asian], mkt, method) is routes.VG
    assert routes.route_of([vanilla()], bs, _mc(hh.LognormalDynamics(), hh.EulerMaruyama())) is routes.PLAIN
    mi = hh.MertonInputs(REF, 0.03, 100.0, 0.2, 0.8, -0.1, 0.15)
    assert routes.route_of([vanilla()], mi, _mc(hh.MertonDynamics(), hh.MertonExact())) is routes.MERTON_LAW
    assert not isinstance(vi, (hh.BlackScholesInputs, hh.MertonInputs, hh.HestonInputs)) and type(vi).__mro__[1] is object


def test_structs_of_a_variance_gamma_solve():
    """both routes: the exact law's dates (r_drift = zero_rate(rate, expiry)), HH_LOGNORMAL + HH_EXACT_LAW, the steps of the
    configuration, θ and ν in hh_vg"""
    curve = hh.RateCurve(REF, [0.5, 2.0], zeros=[0.01, 0.04])
    vi = hh.VarianceGammaInputs(REF, curve, 100.0, 0.2, -0.3, 0.5)
    for route, steps in ((routes.VG_LAW, 1), (routes.VG, 12)):
        model, c, (g,) = route.form_structs(vanilla(105.0), vi, _mc(steps=steps, compat_sqrt_alpha=True))
        assert (c.dynamics, c.strategy, c.n_steps, c.n_partials, c.compat_sqrt_alpha) == (vc.GBM, vc.EXACT, steps, 0, 0)
        assert model.r_drift == hh.zero_rate(curve, EXP) and model.T == hh.yearfrac(REF, EXP) and model.sigma == 0.2
        assert model.discount == hh.df(curve, EXP) and (g.theta, g.nu) == (-0.3, 0.5)
    assert routes.VG_LAW.entry == "hh_mc_solve_vg" and routes.VG_LAW.law and routes.VG.entry == "hh_mc_solve_path_vg"


def test_basket_grouping(monkeypatch):
    """the payoffs of an expiry share one path simulation: path groups first, the vanillas of an expiry ride along or form a
    group of their own; a basket of one European vanilla is the law at expiry"""
    from hedgehog_jl_amd import basket as hb
    vi = vg_inputs()
    later = hh.Date(2023, 1, 1)
    payoffs = [hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2)), vanilla(95.0),
               hh.DigitalOption(101.0, EXP, hh.Put()), vanilla(110.0, hh.Put(), later), vanilla(90.0, None, later),
               hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(2))]
    calls = []

    def fake_paths(group, market_inputs, method, ensemble=True, route=None):
        calls.append(("path", [payoffs.index(p) for p in group], route.name))
        return [hh.MonteCarloSolution(hh.PricingProblem(p, market_inputs), method, 0.0) for p in group]

    def fake_solve(prob, method, ensemble=True):
        calls.append(("solve", prob.payoff.strike))
        return hh.MonteCarloSolution(prob, method, 0.0)

    monkeypatch.setattr(hb, "solve_path_payoffs", fake_paths)
    monkeypatch.setattr(hb, "solve_montecarlo", fake_solve)
    sol = hh.solve(hh.BasketPricingProblem(payoffs, vi), _mc())
    assert calls == [("path", [0, 1, 2, 5], "Variance Gamma paths"), ("path", [3, 4], "Variance Gamma paths")]
    assert all(s is not None for s in sol.solutions)
    calls.clear()
    hh.solve(hh.BasketPricingProblem([vanilla(95.0)], vi), _mc())
    assert calls == [("solve", 95.0)]


def test_fd_lenses_set_theta_and_nu():
    """the lens machinery is generic: SpotLens, VolLens and an optic on θ or ν bump a copy of the VarianceGammaInputs"""
    prob = hh.PricingProblem(vanilla(), vg_inputs())
    up = hh.set(prob, hh.optic("market_inputs.nu"), 0.6)
    assert up.market_inputs.nu == 0.6 and prob.market_inputs.nu == 0.5 and isinstance(up.market_inputs, hh.VarianceGammaInputs)
    assert hh.optic("market_inputs.theta")(prob) == -0.3 and hh.set(prob, hh.optic("market_inputs.theta"), -0.2).market_inputs.theta == -0.2
    assert hh.set(prob, hh.SpotLens(), 101.0).market_inputs.spot == 101.0
    vol = hh.VolLens(100.0, EXP)
    assert vol(prob) == 0.2 and hh.set(prob, vol, 0.25).market_inputs.sigma.σ == 0.25
    # a central difference through the host integral: more kurtosis cheapens the at-the-money call
    g = hh.solve(hh.GreekProblem(prob, hh.optic("market_inputs.nu")), hh.FiniteDifference(1e-4), hh.VarianceGammaAnalytic())
    h, T = 1e-4 * 0.5, hh.yearfrac(REF, EXP)
    want = (vc.mixing_price(dict(vc.BASE, T=T, nu=0.5 + h), 100.0, 1.0) - vc.mixing_price(dict(vc.BASE, T=T, nu=0.5 - h), 100.0, 1.0)) / (2 * h)
    assert g.greek == pytest.approx(float(want), rel=1e-7)
