"""The Crank–Nicolson pricer on the host side, without a GPU: the entry point declared, exported and bound; the scalars
`fd_inputs` hands over; routing and refusals; the scheme itself (tests/fd_cases.py's serial restatement) against the
closed form and the tree; csrc/hh_fd.h as a stand-alone host program (also under AddressSanitizer and UBSan) inside
the bars of the 50-digit run; the committed 50-digit results and their maker."""
import ctypes as C
import importlib.util
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi, pde  # noqa: E402
from oracle import analytic  # noqa: E402
from tests import fd_cases as fc  # noqa: E402
from tests.conftest import host_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hedgehog_mc.h")
REF, EXP = hh.Date(2020, 1, 1), hh.Date(2021, 1, 1)
GOLD = fc.load_golden()


def vanilla(K=100.0, ex=None, cp=None, und=None, expiry=EXP):
    return hh.VanillaOption(K, expiry, ex or hh.American(), cp or hh.Put(), und or hh.Spot())


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------

def test_prototype_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"\bint\s+hh_fd_solve\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert proto and len(proto.group(1).split(",")) == 16
    bound = {s[0]: s for s in _ffi.SYMBOLS}["hh_fd_solve"]
    assert bound[1] is C.c_int and len(bound[2]) == 16
    lib = _ffi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    assert "hh_fd_solve" in {line.split()[-1] for line in nm.stdout.splitlines()} and lib.hh_fd_solve is not None
    assert re.search(r"#define HH_ABI_VERSION 6\b", hdr) and lib.hh_abi_version() == 6
    for name, val in (("HH_FD_MAX_SPACE", 4096), ("HH_FD_MAX_TIME", 65536), ("HH_FD_FORM_A_MAX_SPACE", 1024)):
        assert re.search(rf"#define {name}\s+{val}\b", hdr) and getattr(_ffi, name) == val
    assert re.search(r"enum hh_fd_style \{ HH_FD_EUROPEAN = 0, HH_FD_AMERICAN = 1 \}", hdr)
    assert (_ffi.HH_FD_EUROPEAN, _ffi.HH_FD_AMERICAN) == (0, 1) == (fc.EUROPEAN, fc.AMERICAN)
    assert '"hh_fd.hip"' in open(os.path.join(ROOT, "hedgehog.jl_amd", "_build.py")).read()
    # the header the host program includes names nothing of HIP
    text = open(os.path.join(ROOT, "hedgehog.jl_amd", "csrc", "hh_fd.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__shfl" not in text


# ---- the scalars --------------------------------------------------------------------------------------------------------

def test_fd_inputs_scalars():
    curve = hh.RateCurve(REF, [0.25, 0.5, 1.0, 2.0], zeros=[0.01, 0.02, 0.04, 0.05])
    m = hh.BlackScholesInputs(REF, curve, 100.0, 0.25)
    later = hh.Date(2021, 8, 15)
    payoffs = [vanilla(90.0), vanilla(110.0, hh.European(), hh.Call(), hh.Forward(), later), vanilla(100.0, hh.European()),
               vanilla(120.0, hh.American(), hh.Call(), expiry=later)]
    meth = hh.CrankNicolsonMethod(200, 100, n_std=5.0)
    inp = hh.fd_inputs(payoffs, m, meth)
    assert isinstance(inp, pde.FDInputs)
    for k, p in enumerate(payoffs):
        T = hh.yearfrac(REF, p.expiry)
        r = hh.zero_rate(curve, p.expiry)
        assert (inp.spots[k], inp.strikes[k], inp.sigmas[k], inp.rates[k], inp.expiries[k]) == (100.0, p.strike, 0.25, r, T)
        assert inp.cps[k] == (1.0 if isinstance(p.call_put, hh.Call) else -1.0)
        assert inp.half_widths[k] == 5.0 * 0.25 * math.sqrt(T) + abs(math.log(p.strike / 100.0)) + abs(r - 0.5 * 0.25 * 0.25) * T
        assert inp.half_widths[k] == fc.half_width(100.0, p.strike, r, 0.25, T, 5.0)
    assert inp.styles.tolist() == [1, 0, 0, 1] and inp.styles.dtype == np.int32
    assert inp.rates[0] != inp.rates[1]   # the zero rate of each option's own expiry
    assert (meth.rannacher, hh.CrankNicolsonMethod(8, 4).n_std, meth.device) == (2, 6.0, 0)
    # the operator as the header forms it
    h = inp.half_widths[0] / 100
    lo, di, up = pde.operator(0.25, inp.rates[0], h)
    a, b = 0.25 * 0.25 / 2, inp.rates[0] - 0.25 * 0.25 / 2
    assert lo == pytest.approx(a / h ** 2 - b / (2 * h), rel=1e-14) and up == pytest.approx(a / h ** 2 + b / (2 * h), rel=1e-14)
    assert di == pytest.approx(-2 * a / h ** 2 - inp.rates[0], rel=1e-14)


def test_dispatch_through_solve_and_the_basket(monkeypatch):
    seen = []

    def fake(inp, M, N, R, device=0):
        seen.append((len(inp.spots), M, N, R, device))
        n = len(inp.spots)
        return np.arange(n) + 0.5, np.arange(n) + 0.25, np.arange(n) + 0.125

    monkeypatch.setattr(pde, "fd_device", fake)
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    p1, p2 = vanilla(), vanilla(90.0, hh.European(), hh.Call(), hh.Forward())
    sol = hh.solve(hh.PricingProblem(p1, m), hh.CrankNicolsonMethod(128, 64, rannacher=3, device=1))
    assert isinstance(sol, hh.PDESolution) and (sol.price, sol.delta, sol.gamma) == (0.5, 0.25, 0.125)
    assert sol.problem == hh.PricingProblem(p1, m) and sol.method.space_steps == 128
    b = hh.solve(hh.BasketPricingProblem([p1, p2], m), hh.CrankNicolsonMethod(64, 10))
    assert isinstance(b, hh.BasketPricingSolution) and [s.price for s in b.solutions] == [0.5, 1.5]
    assert all(isinstance(s, hh.PDESolution) for s in b.solutions) and b.solutions[1].problem == hh.PricingProblem(p2, m)
    g = hh.solve(hh.GreekProblem(hh.PricingProblem(p1, m), hh.SpotLens()), hh.FiniteDifference(1e-3), hh.CrankNicolsonMethod(64, 10))
    assert g.greek == 0.0   # two plain solves, one option each: the fake prices them alike
    assert seen == [(1, 128, 64, 3, 1), (2, 64, 10, 2, 0), (1, 64, 10, 2, 0), (1, 64, 10, 2, 0)]


def test_refusals():
    m = hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2)
    prob = hh.PricingProblem(vanilla(), m)
    for kw in (dict(space_steps=2), dict(space_steps=65), dict(space_steps=_ffi.HH_FD_MAX_SPACE + 2), dict(time_steps=0),
               dict(time_steps=_ffi.HH_FD_MAX_TIME + 1), dict(rannacher=-1), dict(rannacher=65), dict(n_std=0.0),
               dict(n_std=float("nan"))):
        with pytest.raises(ValueError):
            hh.solve(prob, hh.CrankNicolsonMethod(**dict(dict(space_steps=64, time_steps=64), **kw)))
    with pytest.raises(TypeError):
        hh.solve(prob, hh.CrankNicolsonMethod(64.0, 64))
    # a drift the grid cannot carry: the message names the smallest M that can, and that M is accepted
    steep = hh.PricingProblem(vanilla(), hh.BlackScholesInputs(REF, 0.5, 100.0, 0.05))
    with pytest.raises(ValueError, match=r"space_steps >= (\d+)") as e:
        hh.fd_inputs([steep.payoff], steep.market_inputs, hh.CrankNicolsonMethod(8, 10))
    need = int(re.search(r"space_steps >= (\d+)", str(e.value)).group(1))
    inp = hh.fd_inputs([steep.payoff], steep.market_inputs, hh.CrankNicolsonMethod(need, 10))
    lo, _, up = pde.operator(inp.sigmas[0], inp.rates[0], inp.half_widths[0] / (need // 2))
    assert need % 2 == 0 and need > 8 and lo > 0 and up > 0
    lo, _, up = pde.operator(inp.sigmas[0], inp.rates[0], inp.half_widths[0] / ((need - 2) // 2))
    assert not (lo > 0 and up > 0)
    meth = hh.CrankNicolsonMethod(64, 64)
    with pytest.raises(hh.MethodError, match="Forward"):
        hh.solve(hh.PricingProblem(vanilla(und=hh.Forward()), m), meth)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(vanilla(), hh.HestonInputs(REF, 0.05, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7)), meth)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(vanilla(), hh.MertonInputs(REF, 0.03, 100.0, 0.2, 0.8, -0.1, 0.15)), meth)
    with pytest.raises(hh.MethodError):
        hh.solve(hh.PricingProblem(hh.AsianOption(100.0, EXP, hh.Call()), m), meth)
    d = hh.Dual(1.0, (1.0,))
    for dual_prob in (hh.PricingProblem(vanilla(), hh.BlackScholesInputs(REF, 0.05, 100.0 * d, 0.2)),
                      hh.PricingProblem(vanilla(), hh.BlackScholesInputs(REF, 0.05, 100.0, 0.2 * d)),
                      hh.PricingProblem(vanilla(), hh.BlackScholesInputs(REF, 0.05 * d, 100.0, 0.2)),
                      hh.PricingProblem(vanilla(100.0 * d), m)):
        with pytest.raises(hh.MethodError, match="FiniteDifference"):
            hh.solve(dual_prob, meth)
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.ForwardAD(), meth)
    with pytest.raises(hh.MethodError, match="FiniteDifference"):
        hh.solve(hh.BasketPricingProblem([vanilla(), vanilla(100.0 * d, hh.European())], m), meth)


# ---- the scheme -----------------------------------------------------------------------------------------------------------

_restated = {}


def restated(ci, cp, style, M, N):
    """fp64 restatement on the default grid (n_std = 6, R = 2), once per process"""
    key = (ci, cp, style, M, N)
    if key not in _restated:
        _restated[key] = fc.restate(fc.FP64, *fc.scalars((ci, cp, style, M, N, 2, 6.0)))
    return _restated[key]


def black_scholes(ci, cp):
    S0, K, r, sigma, T = fc.CASES[ci]
    payoff = hh.VanillaOption(K, hh.to_ticks(REF) + T * hh.dates.MILLISECONDS_IN_YEAR_365, hh.European(),
                              hh.Call() if cp > 0 else hh.Put(), hh.Spot())
    assert hh.yearfrac(REF, payoff.expiry) == T
    return hh.solve(hh.PricingProblem(payoff, hh.BlackScholesInputs(REF, r, S0, sigma)), hh.BlackScholesAnalytic()).price


@pytest.mark.parametrize("ci", [0, 4, 5])
def test_second_order_convergence_with_the_strike_on_a_node(ci):
    """K = S0: the error against BlackScholesAnalytic falls by 4 per refinement of both steps, ratios in [3.9, 4.1]"""
    for cp in (1.0, -1.0):
        want = black_scholes(ci, cp)
        errs = [abs(restated(ci, cp, fc.EUROPEAN, M, N)[0] - want) for M, N in ((128, 64), (256, 128), (512, 256))]
        ratios = [errs[0] / errs[1], errs[1] / errs[2]]
        print(f"\ncase {ci} cp {cp}: errors {errs}, ratios {ratios}")
        assert all(3.9 <= q <= 4.1 for q in ratios)


@pytest.mark.parametrize("ci", [1, 2, 3])
def test_european_against_the_closed_form_off_the_nodes(ci):
    for cp in (1.0, -1.0):
        want = black_scholes(ci, cp)
        for (M, N), bound in (((256, 128), 1.5e-3), ((512, 256), 3e-4)):
            miss = abs(restated(ci, cp, fc.EUROPEAN, M, N)[0] - want)
            print(f"\ncase {ci} cp {cp} grid {(M, N)}: |restatement − closed form| {miss:.3e}")
            assert miss <= bound


@pytest.mark.parametrize("ci", range(len(fc.CASES)))
def test_american_put_against_the_tree(ci):
    """the numpy tree oracle at 4000 steps: within 1.5e-3 at (512, 256); and the exercise orderings, exactly in fp64"""
    S0, K, r, sigma, T = fc.CASES[ci]
    tree = analytic.crr_price(S0, K, r, sigma, T, 4000, cp=-1.0, american=True)
    got = restated(ci, -1.0, fc.AMERICAN, 512, 256)[0]
    print(f"\ncase {ci}: restatement {got!r}, tree {tree!r}, |diff| {abs(got - tree):.3e}")
    assert abs(got - tree) <= 1.5e-3
    assert got >= restated(ci, -1.0, fc.EUROPEAN, 512, 256)[0] - 1e-12 and got >= K - math.exp(math.log(S0))


# ---- csrc/hh_fd.h as a host program -----------------------------------------------------------------------------------------

HOST_RUNS = [r for r in fc.run_list() if r[3] <= 258]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", ["plain", "asan-ubsan"])
def test_serial_step_host_program(tmp_path, build):
    """tests/c/fd_host_check.cpp — its own main, csrc/hh_fd.h included — prices every run up to M = 258 with the header's
    serial step inside the bars of the 50-digit run, and refuses an operator that is not positive.  Built plainly and
    with -fsanitize=address,undefined, and run as a program: nothing is loaded into this interpreter."""
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-fno-omit-frame-pointer"]
    exe = str(tmp_path / ("fd_host_check_" + build))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                    os.path.join(ROOT, "tests", "c", "fd_host_check.cpp"), "-o", exe], check=True)

    def line(args):
        return " ".join([float(v).hex() for v in args[:7]] + [str(int(v)) for v in args[7:]]) + "\n"

    (tmp_path / "options.txt").write_text("".join(line(fc.scalars(r)) for r in HOST_RUNS))
    run = subprocess.run([exe, str(tmp_path / "options.txt")], capture_output=True, text=True, env=host_env(), timeout=120)
    assert run.returncode == 0, run.stderr
    rows = [[float.fromhex(t) for t in ln.split()] for ln in run.stdout.splitlines()]
    assert len(rows) == len(HOST_RUNS) >= 400
    for r, got in zip(HOST_RUNS, rows):
        exact, e64 = GOLD[r]
        miss = np.array([fc.err(got[k], exact[k]) for k in range(3)])
        assert np.all(miss <= fc.bars(r, e64)), (r, miss.tolist())
    S0, K, r_, sigma, T = fc.CASES[0]
    (tmp_path / "bad.txt").write_text(line((S0, K, -1.0, sigma, 40.0, T, fc.half_width(S0, K, r_, sigma, T), 1, 64, 10, 2)))
    assert subprocess.run([exe, str(tmp_path / "bad.txt")], capture_output=True, env=host_env(), timeout=60).returncode == 3


# ---- the committed 50-digit results ------------------------------------------------------------------------------------

def test_golden_covers_the_runs_and_its_bars_are_fp64_sized():
    runs = fc.run_list()
    assert len(runs) == len(set(runs)) == len(GOLD) and set(runs) == set(GOLD)
    for r in runs:
        exact, e64 = GOLD[r]
        S0, K, _, _, _, _, W, _, M, _, _ = fc.scalars(r)
        A = fc.magnitudes(S0, K, W, M)
        # the fp64 run sits within 1e-9 of the size of the terms each output differences: the bars are rounding-sized
        assert np.all(np.array(e64) <= 1e-9 * A), (r, e64)
        assert np.all(fc.bars(r, e64) >= 20 * fc.EPS * A)
    narrow = [r for r in runs if r[6] == fc.NARROW]
    assert {(r[1], r[2]) for r in narrow} == set(fc.SIDES)


def test_maker_regenerates_a_sample_identically():
    spec = importlib.util.spec_from_file_location("make_fd_exact", os.path.join(ROOT, "tests", "golden", "make_fd_exact.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    import json
    doc = json.load(open(fc.GOLDEN))
    assert doc["dps"] == fc.DPS and [tuple(c) for c in doc["cases"]] == fc.CASES
    by = {(r["case"], r["cp"], r["style"], r["M"], r["N"], r["R"], r["n_std"]): r for r in doc["runs"]}
    sample = [r for r in fc.run_list() if r[3] <= 66 and r[4] <= 3][::7] + [(0, -1.0, 1, 64, 50, 2, fc.NARROW)]
    assert len(sample) >= 10
    for r in sample:
        assert json.loads(json.dumps(maker.record(r))) == by[r], r


def test_each_mutation_moves_the_restatement_beyond_the_bars():
    """the five ways to get the scheme wrong that the device test must notice: each moves some output of some committed
    run by more than that run's bar (on the device test's own runs, so a device that carried the mutation would fail)"""
    runs = [r for r in fc.run_list() if r[3] <= 66 and r[4] == 50]
    for mutation in fc.MUTATIONS:
        moved = 0
        for r in runs:
            exact, e64 = GOLD[r]
            got = fc.restate(fc.FP64, *fc.scalars(r), mutation=mutation)
            moved += bool(np.any(np.array([fc.err(got[k], exact[k]) for k in range(3)]) > fc.bars(r, e64)))
        print(f"\n{mutation}: moves {moved} of {len(runs)} runs beyond their bars")
        assert moved > 0, mutation
