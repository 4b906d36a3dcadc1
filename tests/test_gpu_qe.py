"""Heston paths by the quadratic-exponential scheme on the device (hh_qe.hip) — hh_mc_path_stats_qe, hh_mc_solve_path_qe
and the Python route above them.

  * PATH BY PATH against the restatement of tests/qe_cases.py at 50 digits on the draws the device makes itself (the
    oracle's host Philox, the normals restated by hh_rng.h's formulas): the five rows and var_T of every member within
    euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A).  257 trajectories (two workgroups, a one-lane tail), two
    models whose trajectories take both branches and both arms of U within a case on more than one step (the fixture
    records the counts; on one step every member starts at V0 and shares one ψ — "feller" is quadratic there,
    "low_v0" exponential with both arms).  A wrong branch moves a state by far more than a bar.
  * IDENTITIES, bit for bit: trajectory i does not depend on the size of the call; a payoff's result does not depend on
    its neighbours; path_values are the payoffs of the returned statistics.
  * THE LAW, fixed seeds, 2¹⁸ trajectories: calls within 4 standard errors of Carr–Madan where Euler–Maruyama on the
    same 16 steps is more than 10 away; the mean of var_T against θ + (v₀ − θ)e^{−κT}; the martingale correction.
  * Errors: every HH_ERR_INVALID / HH_ERR_UNSUPPORTED case of the header, with its text, without a launch.
The module prints its worst error/bar per row at its end (`-s`)."""
import ctypes as C
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import carr_madan_cases as cmc  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import path_bridge_cases as bc  # noqa: E402
from tests import path_payoff_cases as pc  # noqa: E402
from tests import qe_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

DOC = qc.load_golden()
MONITORED = _ffi.HH_EXTREMES_MONITORED
ROW_NAMES = ("SUM_S", "SUM_X", "MAX_S", "MIN_S", "S_T", "var_T")
_cache = {}


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("quadratic-exponential (device)")
    yield w
    w.report()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def path_stats(ctx, m, q, c, every, start, want_var=True):
    stats, var = np.empty((_ffi.HH_PATH_STATS, n_total(c))), (np.empty(n_total(c)) if want_var else None)
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_qe(ctx.handle, C.byref(m), C.byref(q), C.byref(c), every, start, stats.ctypes.data, 0,
                                          var.ctypes.data if want_var else None, C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return stats, var


def solve_path(ctx, m, q, c, every, start, payoffs, want=True, want_var=False):
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = (np.empty((K, n_total(c))), np.empty((_ffi.HH_PATH_STATS, n_total(c)))) if want else (None, None)
    var = np.empty(n_total(c)) if want_var else None
    ctx.check(ctx.lib.hh_mc_solve_path_qe(ctx.handle, C.byref(m), C.byref(q), C.byref(c), every, start, arr, K, res,
                                          values.ctypes.data if want else None, stats.ctypes.data if want else None,
                                          var.ctypes.data if want_var else None))
    return list(res), values, stats, var


def same_result(a, b):
    return (a.price, a.std_error, a.sum_payoff, a.sumsq_payoff, a.n_paths_done) == \
        (b.price, b.std_error, b.sum_payoff, b.sumsq_payoff, b.n_paths_done)


def law_seeds(n, salt=3):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt)


def payoff_list():
    return [pc.payoff(pc.VANILLA, 100.0, 1.0), pc.payoff(pc.ARITH, 98.0, 1.0), pc.payoff(pc.GEOM, 101.0, -1.0),
            pc.payoff(pc.BARRIER, 95.0, 1.0, pc.DOWN_OUT, 80.0, 1.5), pc.payoff(pc.DCASH, 102.0, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 99.0, -1.0), pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0),
            pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FIXED, 100.0, 1.0)]


# ---- (a) path by path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("include_start", [0, 1])
@pytest.mark.parametrize("shape", qc.PATH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(qc.MODELS))
def test_path_by_path(hhlib, oracle, worst, name, shape, include_start, anti, mart):
    n_steps, every = shape
    case, seeds = qc.MODELS[name], qc.path_seeds()
    rec = next(b for b in DOC["branches"] if b["model"] == name and b["n_steps"] == n_steps)
    if n_steps > 1:
        assert rec["quadratic"] > 0 and rec["exponential"] > rec["zero"] > 0
    Z = cached(("Z", n_steps), lambda: qc.step_normals(oracle, seeds, n_steps))
    U = cached(("U", n_steps), lambda: qc.step_uniforms(oracle, seeds, n_steps))
    runs = cached(("runs", name, n_steps, mart), lambda: qc.walks(case, n_steps, Z, U, 1, mart)[0])
    ref = qc.reference(case, runs[:2 if anti else 1], every, include_start)
    bars = etc.path_bar(ref["e64"], ref["A"])
    stats, var = path_stats(hhlib, qc.model_of(case), _ffi.make_qe(0.0, mart), qc.config_of(qc.PATH_N, n_steps, seeds, anti),
                            every, include_start)
    got = np.vstack([stats, var[None, :]])
    bad = []
    for mem in range(ref["members"]):
        for i in range(qc.PATH_N):
            for row in range(6):
                bad.append(worst.check(ROW_NAMES[row], got[row][mem * qc.PATH_N + i], ref["want"][mem][i][row],
                                       bars[mem][i][row], f"{name} {n_steps}x{every} start={include_start} anti={anti} "
                                       f"mart={mart} member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ---- (b) identities, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
def test_one_wave_and_many(hhlib, anti):
    """n_paths of 1, 63, 64, 65, 256 and 513 on 3 steps: trajectory i of every size == trajectory i of the largest"""
    case, big = qc.MODELS["feller"], 513
    seeds = law_seeds(big, 17)
    m, q = qc.model_of(case), _ffi.make_qe(0.0, 1)
    whole, wvar = path_stats(hhlib, m, q, qc.config_of(big, 3, seeds, anti), 1, 1)
    assert np.all(np.isfinite(whole)) and np.all(wvar >= 0.0)
    for n in (1, 63, 64, 65, 256, 513):
        stats, var = path_stats(hhlib, m, q, qc.config_of(n, 3, seeds[:n], anti), 1, 1)
        for mem in range(2 if anti else 1):
            assert np.array_equal(stats[:, mem * n:(mem + 1) * n], whole[:, mem * big:mem * big + n]), (n, mem)
            assert np.array_equal(var[mem * n:(mem + 1) * n], wvar[mem * big:mem * big + n]), (n, mem)


def test_payoff_independence_and_path_values(hhlib):
    """result k of a 16-payoff call == the one-payoff call; path_values rows == the payoffs of the returned statistics"""
    case = qc.MODELS["low_v0"]
    n, n_steps, every, start = 3000, 6, 2, 1
    m, q = qc.model_of(case), _ffi.make_qe(0.0, 0)
    c = qc.config_of(n, n_steps, law_seeds(n, 29), 1)
    payoffs = payoff_list() + [pc.payoff(pc.VANILLA, 70.0 + 10.0 * k, 1.0 if k % 2 else -1.0) for k in range(8)]
    assert len(payoffs) == 16
    together, values, stats, _ = solve_path(hhlib, m, q, c, every, start, payoffs)
    plain, _ = path_stats(hhlib, m, q, c, every, start, want_var=False)
    assert np.array_equal(plain, stats)
    n_mon = pc.n_mon(n_steps, every, start)
    for k, p in enumerate(payoffs):
        alone, _, _, _ = solve_path(hhlib, m, q, c, every, start, [p], want=False)
        assert same_result(alone[0], together[k]), k
        want = bc.payoff_from_stats(stats, p, n_mon, MONITORED)
        if p.kind == pc.GEOM:  # numpy's exp against the device's
            np.testing.assert_allclose(values[k], want, rtol=1e-14, atol=1e-13)
        else:
            assert np.array_equal(values[k], want), k
        pair = (values[k][:n] + values[k][n:]) / 2
        assert together[k].sum_payoff == pytest.approx(math.fsum(pair), rel=1e-13, abs=1e-12)
        assert together[k].n_paths_done == n


# ---- (c) the law ---------------------------------------------------------------------------------------------------------------

N_LAW = 2 ** 18


def carr_madan_calls(ctx, case, strikes):
    """hh_carr_madan_basket on the case, α and bound of tests/carr_madan_cases.py's Feller-violating Heston case"""
    _, ref = cmc.BY_ID["feller_violated"]
    K = np.array(strikes)
    n = len(K)
    D = math.exp(-case["r_drift"] * case["T"])
    arrs = [K, np.ones(n), np.full(n, case["T"]), np.full(n, case["r_drift"]), np.full(n, D)]
    out = np.empty(n)
    m = qc.model_of(dict(case, discount=D))
    ctx.check(ctx.lib.hh_carr_madan_basket(ctx.handle, C.byref(m), _ffi.HH_HESTON, 0, ref["alpha"], ref["bound"],
                                           *[a.ctypes.data for a in arrs], n, out.ctypes.data))
    return out


def test_the_law_against_carr_madan_where_euler_is_biased(hhlib):
    """κ = 0.3, θ = v₀ = 0.04, σ = 0.9, ρ = −0.5, T = 5 on 16 steps, expiry-only: QE calls at K = 70, 100, 140 within 4
    standard errors of Carr–Madan (the scheme's own bias there is <= 0.02 against a standard error of about 0.05);
    Euler–Maruyama (em_split = 1) at K = 100 on the same steps and seeds is more than 10 standard errors away."""
    case, strikes = qc.LAW, [70.0, 100.0, 140.0]
    want = carr_madan_calls(hhlib, case, strikes)
    assert want[1] == pytest.approx(9.3287, abs=2e-4)  # the issue's Gil-Pelaez figure: the reference is the model's price
    seeds = law_seeds(N_LAW)
    m = qc.model_of(dict(case, discount=1.0))
    payoffs = [pc.payoff(pc.VANILLA, K, 1.0) for K in strikes]
    res, _, _, _ = solve_path(hhlib, m, _ffi.make_qe(0.0, 0), qc.config_of(N_LAW, 16, seeds), 16, 0, payoffs, want=False)
    for r, w, K in zip(res, want, strikes):
        miss = (r.price - w) / r.std_error
        print(f"\nQE K={K:g}: price {r.price:.5f}, Carr–Madan {w:.5f}, {miss:+.2f} standard errors of {r.std_error:.4f}")
        assert r.std_error > 0.0 and abs(miss) <= 4.0, (K, r.price, w, r.std_error)
    ce = _ffi.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, N_LAW, 16, em_split=1, seeds=seeds)
    arr, out = (_ffi.hh_path_payoff * 1)(payoffs[1]), (_ffi.hh_result * 1)()
    hhlib.check(hhlib.lib.hh_mc_solve_path(hhlib.handle, C.byref(m), C.byref(ce), 16, 0, arr, 1, out, None, None))
    miss = (out[0].price - want[1]) / out[0].std_error
    print(f"\nEuler K=100: price {out[0].price:.5f}, {miss:+.2f} standard errors of {out[0].std_error:.4f}")
    assert abs(miss) > 10.0


@pytest.mark.parametrize("n_steps", [4, 8, 16])
def test_exact_mean_of_the_variance(hhlib, n_steps):
    """the scheme matches the conditional mean exactly, so E v_T = θ + (v₀ − θ)e^{−κT} on any number of steps; v₀ = 0.001
    so that the mean moves"""
    case = qc.MODELS["low_v0"]
    _, var = path_stats(hhlib, qc.model_of(case), _ffi.make_qe(0.0, 0), qc.config_of(N_LAW, n_steps, law_seeds(N_LAW, 7)),
                        n_steps, 0)
    want = case["theta"] + (case["V0"] - case["theta"]) * math.exp(-case["kappa"] * case["T"])
    se = var.std(ddof=1) / math.sqrt(N_LAW)
    miss = (var.mean() - want) / se
    print(f"\nmean var_T on {n_steps} steps: {var.mean():.6f}, exact {want:.6f}, {miss:+.2f} standard errors")
    assert np.all(var >= 0.0) and abs(miss) <= 4.0


def test_the_martingale_correction(hhlib):
    """κ = 0.5, θ = v₀ = 0.04, σ = 1, ρ = −0.9, T = 10, r = 0 on 8 steps: with the correction the mean of S_T is within 4
    standard errors of S0; without it, more than 6 above"""
    case, n_steps = qc.DRIFTY, 8
    m, c = qc.model_of(case), qc.config_of(N_LAW, n_steps, law_seeds(N_LAW, 11))
    out = {}
    for mart in (1, 0):
        stats, _ = path_stats(hhlib, m, _ffi.make_qe(0.0, mart), c, n_steps, 0, want_var=False)
        S = stats[pc.S_T]
        out[mart] = (S.mean() - case["S0"]) / (S.std(ddof=1) / math.sqrt(N_LAW))
        print(f"\nmartingale={mart}: mean S_T {S.mean():.4f}, {out[mart]:+.2f} standard errors from S0")
    assert abs(out[1]) <= 4.0 and out[0] > 6.0


def test_antithetic_pairs_reduce_the_standard_error(hhlib):
    case, n = qc.MODELS["feller"], 2 ** 16
    m, q, seeds = qc.model_of(case), _ffi.make_qe(0.0, 0), law_seeds(2 ** 16, 13)
    pay = [pc.payoff(pc.VANILLA, 100.0, 1.0)]
    plain, _, _, _ = solve_path(hhlib, m, q, qc.config_of(n, 8, seeds, 0), 8, 0, pay, want=False)
    anti, _, _, _ = solve_path(hhlib, m, q, qc.config_of(n, 8, seeds, 1), 8, 0, pay, want=False)
    print(f"\nstandard error plain {plain[0].std_error:.5f}, antithetic {anti[0].std_error:.5f}")
    assert 0.0 < anti[0].std_error < plain[0].std_error
    assert abs(anti[0].price - plain[0].price) <= 4.0 * plain[0].std_error


# ---- (d) errors ------------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")


def test_errors_come_back_without_a_launch(hhlib):
    ctx = hhlib
    case = qc.MODELS["feller"]
    n, steps = 300, 4
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    good_m, good_q = qc.model_of(case), _ffi.make_qe(0.0, 0)
    outs = (_ffi.hh_result * 1)()
    pay = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.VANILLA, 100.0, 1.0))
    stats = np.empty((5, n))
    cfg = lambda **kw: qc.config_of(n, steps, seeds, **kw)  # noqa: E731

    def both(mm, qq, cc, every=1):
        """-> the two entry points' (return code, text)"""
        a = ctx.lib.hh_mc_solve_path_qe(ctx.handle, mm, qq, cc, every, 0, pay, 1, outs, None, None, None)
        ta = ctx.lib.hh_last_error(ctx.handle).decode()
        b = ctx.lib.hh_mc_path_stats_qe(ctx.handle, mm, qq, cc, every, 0, stats.ctypes.data, 0, None, None)
        return (a, ta), (b, ctx.lib.hh_last_error(ctx.handle).decode())

    def expect(mm, qq, cc, code, text, **kw):
        for who, (rc, msg) in zip(("hh_mc_solve_path_qe", "hh_mc_path_stats_qe"), both(mm, qq, cc, **kw)):
            assert rc == code and text in msg and who in msg, (who, rc, code, text, msg)

    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
        bad_models = [dict(kappa=0.0), dict(kappa=-1.0), dict(theta=0.0), dict(theta=-0.04), dict(sigma=0.0), dict(sigma=-0.5),
                      dict(V0=-1e-9)]
        for d in bad_models:
            expect(C.byref(qc.model_of(dict(case, **d))), C.byref(good_q), C.byref(cfg()), INV, "kappa, theta, sigma must be > 0 and V0 >= 0")
        for d in (dict(rho=1.0000001), dict(rho=-1.5), dict(kappa=NAN), dict(theta=INF), dict(V0=NAN), dict(sigma=NAN),
                  dict(rho=NAN), dict(r_drift=INF), dict(T=INF), dict(S0=-1.0), dict(T=0.0)):
            expect(C.byref(qc.model_of(dict(case, **d))), C.byref(good_q), C.byref(cfg()), INV, "model scalars finite")
        for psi in (0.5, 0.999999, 2.0000001, -1.0, NAN, INF):
            expect(C.byref(good_m), C.byref(_ffi.make_qe(psi, 0)), C.byref(cfg()), INV, "psi_c must be 0 (the default 1.5) or lie in [1, 2]")
        expect(C.byref(qc.model_of(dict(case, kappa=1e-20, sigma=1e-8))), C.byref(good_q), C.byref(cfg()), INV, "rounds to 0")
        expect(C.byref(qc.model_of(dict(case, sigma=100.0, theta=1e-6))), C.byref(good_q), C.byref(cfg()), INV, "is above HH_QE_MAX_PSI")
        expect(C.byref(good_m), None, C.byref(cfg()), INV, "NULL argument")
        expect(None, C.byref(good_q), C.byref(cfg()), INV, "NULL argument")
        expect(C.byref(good_m), C.byref(good_q), None, INV, "NULL argument")
        expect(C.byref(good_m), C.byref(good_q), C.byref(cfg()), INV, "must be >= 1 and divide n_steps", every=3)
        expect(C.byref(good_m), C.byref(good_q), C.byref(qc.config_of(0, steps, seeds)), INV, "1 <= n_paths")
        # unsupported
        for dyn, strat in ((_ffi.HH_LOGNORMAL, _ffi.HH_QE), (_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA),
                           (_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA), (_ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW)):
            expect(C.byref(good_m), C.byref(good_q), C.byref(_ffi.make_config(dyn, strat, n, steps, seeds=seeds)), UNS,
                   "needs HestonDynamics + the quadratic-exponential strategy (HH_QE)")
        expect(C.byref(good_m), C.byref(good_q), C.byref(cfg(noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4))), UNS, "GENERATE noise, no dual partials")
        expect(C.byref(good_m), C.byref(good_q), C.byref(cfg(n_partials=2)), UNS, "GENERATE noise, no dual partials")
        expect(C.byref(qc.model_of(dict(case, rho=0.9))), C.byref(_ffi.make_qe(0.0, 1)), C.byref(cfg()), UNS, "run without it")
        # HH_QE is refused by the entry points of the other strategies
        res = _ffi.hh_result()
        assert ctx.lib.hh_mc_solve(ctx.handle, C.byref(good_m), C.byref(cfg()), C.byref(res), None) == UNS
        assert ctx.lib.hh_mc_solve_path(ctx.handle, C.byref(good_m), C.byref(cfg()), 1, 0, pay, 1, outs, None, None) == UNS
        assert ctx.read_timings() == []  # nothing was launched
        # the edges are admitted, ρ > 0 without the correction too, and the context solves
        for psi in (1.0, 2.0):
            res, _, st, var = solve_path(ctx, good_m, _ffi.make_qe(psi, 1), cfg(), 2, 1, [pc.payoff(pc.VANILLA, 100.0, 1.0)], want_var=True)
            assert np.all(np.isfinite(st)) and np.all(var >= 0.0) and res[0].price > 0.0 and res[0].n_paths_done == n
        st, var = path_stats(ctx, qc.model_of(dict(case, rho=0.9, V0=0.0)), good_q, cfg(anti=1), 1, 0)
        assert np.all(np.isfinite(st)) and np.all(var >= 0.0)
        assert len(ctx.read_timings()) == 5  # two slots per solve, one for the statistics alone
    finally:
        ctx.enable_timing(False)


# ---- (e) the Python route --------------------------------------------------------------------------------------------------

def test_python_route_gives_the_c_calls_numbers(hhlib):
    ref, exp_ = hh.Date(2021, 1, 1), hh.Date(2024, 1, 1)
    case = qc.LAW
    mkt = hh.HestonInputs(ref, 0.0, case["S0"], case["V0"], case["kappa"], case["theta"], case["sigma"], case["rho"])
    n, steps = 4096, 12
    seeds = law_seeds(n, 23)
    for strat, anti in ((hh.HestonQE(), False), (hh.HestonQE(psi_c=1.2, martingale=True), True)):
        vr = hh.Antithetic() if anti else hh.NoVarianceReduction()
        method = hh.MonteCarlo(hh.HestonDynamics(), strat, hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=vr))
        vanilla = hh.VanillaOption(105.0, exp_, hh.European(), hh.Call(), hh.Spot())
        asian = hh.AsianOption(100.0, exp_, hh.Call(), monitoring=hh.Monitoring(3))
        out = hh.BarrierOption(100.0, 70.0, exp_, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(3))
        m = qc.model_of(dict(case, T=hh.yearfrac(ref, exp_), discount=1.0))
        q = _ffi.make_qe(strat.psi_c, strat.martingale)
        c = qc.config_of(n, steps, seeds, int(anti))
        for payoff, packed, every in ((vanilla, pc.payoff(pc.VANILLA, 105.0, 1.0), steps), (asian, pc.payoff(pc.ARITH, 100.0, 1.0), 3),
                                      (out, pc.payoff(pc.BARRIER, 100.0, 1.0, pc.DOWN_OUT, 70.0, 0.0), 3)):
            sol = hh.solve(hh.PricingProblem(payoff, mkt), method)
            res, _, stats, _ = solve_path(hhlib, m, q, c, every, 0, [packed])
            assert sol.price == res[0].price and sol.std_error == res[0].std_error and sol.price > 0.0, type(payoff).__name__
            assert np.array_equal(sol.ensemble, stats)
        basket = hh.solve(hh.BasketPricingProblem([asian, vanilla, out], mkt), method)
        for p, s in zip((asian, vanilla, out), basket.solutions):
            assert s.price == hh.solve(hh.PricingProblem(p, mkt), method).price
