"""Multilevel Monte Carlo on the device (hh_mc_path_stats_coupled, hh_mc_solve_path_coupled; csrc/hh_path.hip) and through
hh.solve (hedgehog.jl_amd/mlmc.py).

(1) the fine leg is the plain solve, bit for bit; (2) the coarse leg is the plain REPLAY solve on the summed increments,
bit for bit; (3) under lognormal dynamics the two legs agree up to rounding; (4) the payoff differences against the numpy
restatement and exact sums, and a payoff's result does not depend on what else is in the call; (5) the refusals;
(6) the telescoping sum against a single-level solve on the finest grid; (7) the coupling reduces the variance as the
restatement of tests/mlmc_cases.py says it does; (8) the adaptive form.  Shapes: 700 trajectories are three workgroups of
the statistics kernel, the last ragged; 2 steps is the smallest coupled level (one coarse step)."""
import ctypes as C
import math

import numpy as np
import pytest

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi
from tests import mlmc_cases as mc
from tests import path_bridge_cases as bc
from tests import path_payoff_cases as pc

pytestmark = pytest.mark.gpu

LOGN, HEST, EULER = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA
INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
MODELS = {"heston-split": (HEST, 1), "heston-classic": (HEST, 0), "lognormal": (LOGN, 1)}
N = 700
SHAPES = [(2, 2), (6, 2), (6, 6), (16, 4)]  # (n_steps, monitor_every)
ROWS = _ffi.HH_PATH_STATS


def seeds_for(n):
    return np.random.default_rng(20240911).integers(0, 2**64, size=n, dtype=np.uint64)


def config(dyn, n, steps, split=1, **kw):
    return _ffi.make_config(dyn, EULER, n, steps, em_split=split, seeds=seeds_for(n), **kw)


def coupled_stats(ctx, m, c, every, start):
    stats = np.empty((ROWS, 2 * int(c.n_paths)))
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_coupled(ctx.handle, C.byref(m), C.byref(c), every, start, stats.ctypes.data, 0, C.byref(res)))
    assert res.n_paths_done == c.n_paths and res.kernel_ms > 0.0
    return stats


def coupled_solve(ctx, m, c, every, start, payoffs):
    """-> (out_diff, out_fine, path_values (K, 2n), statistics (5, 2n))"""
    K, n = len(payoffs), int(c.n_paths)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    diff, fine = (_ffi.hh_result * K)(), (_ffi.hh_result * K)()
    values, stats = np.empty((K, 2 * n)), np.empty((ROWS, 2 * n))
    ctx.check(ctx.lib.hh_mc_solve_path_coupled(ctx.handle, C.byref(m), C.byref(c), every, start, arr, K, diff, fine,
                                               values.ctypes.data, stats.ctypes.data))
    return list(diff), list(fine), values, stats


def plain_stats(ctx, m, c, every, start):
    stats = np.empty((ROWS, int(c.n_paths)))
    ctx.check(ctx.lib.hh_mc_path_stats(ctx.handle, C.byref(m), C.byref(c), every, start, stats.ctypes.data, 0, None))
    return stats


def every_kind(stats):
    """one payoff of each kind 0 … 7; the barrier is exactly one trajectory's maximum (a touch)"""
    up = float(np.sort(stats[pc.MAX_S])[stats.shape[1] // 2])
    return [pc.payoff(pc.VANILLA, 100.0, 1.0), pc.payoff(pc.ARITH, 100.0, -1.0), pc.payoff(pc.GEOM, 99.0, 1.0),
            pc.payoff(pc.BARRIER, 100.0, 1.0, pc.UP_OUT, up, rebate=1.25), pc.payoff(pc.DCASH, 101.0, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 100.0, -1.0), pc.payoff(bc.LB_FLOAT, 0.0, 1.0), pc.payoff(bc.LB_FIXED, 102.0, -1.0)]


def same_result(a, b):
    return (a.price, a.std_error, a.sum_payoff, a.sumsq_payoff, a.n_paths_done) == \
        (b.price, b.std_error, b.sum_payoff, b.sumsq_payoff, b.n_paths_done)


# ---- (1) the fine leg is the plain solve -------------------------------------------------------------------------------

@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("name", list(MODELS))
def test_fine_leg_is_the_plain_solve(hhlib, name, start):
    dyn, split = MODELS[name]
    m = _ffi.make_model(sigma=0.2) if dyn == LOGN else _ffi.make_model()
    for steps, every in SHAPES:
        c = config(dyn, N, steps, split)
        plain = plain_stats(hhlib, m, c, every, start)
        np.testing.assert_array_equal(coupled_stats(hhlib, m, c, every, start)[:, :N], plain, err_msg=str((name, steps, every)))
        payoffs = every_kind(plain)
        K = len(payoffs)
        want = (_ffi.hh_result * K)()
        hhlib.check(hhlib.lib.hh_mc_solve_path_ex(hhlib.handle, C.byref(m), C.byref(c), every, start, bc.MONITORED,
                                                  (_ffi.hh_path_payoff * K)(*payoffs), K, want, None, None))
        _, fine, _, stats = coupled_solve(hhlib, m, c, every, start, payoffs)
        np.testing.assert_array_equal(stats[:, :N], plain)
        for k in range(K):
            assert same_result(fine[k], want[k]), (name, steps, every, start, k)
            assert fine[k].n_paths_done == N


# ---- (2) the coarse leg is the plain solve on the summed increments ---------------------------------------------------------

def summed_increments(ctx, dyn, m, n, fine_steps):
    """hh_wiener_fill's increments of the fine grid, pairs added (one rounded addition each): [tile][coarse step][comp][256]"""
    nc = 2 if dyn == HEST else 1
    elems = ctx.lib.hh_replay_elems(n, fine_steps, dyn)
    buf = _ffi.DeviceBuffer(ctx, 8 * elems)
    seeds = seeds_for(n)  # (held here: the call reads the host array)
    ctx.check(ctx.lib.hh_wiener_fill(ctx.handle, dyn, m.rho, m.T, fine_steps, n, seeds.ctypes.data, 0, buf.ptr))
    fine = buf.download(np.empty(elems)).reshape(-1, fine_steps, nc, 256)
    buf.free()
    return fine[:, 0::2] + fine[:, 1::2]


def replay_terminal(ctx, dyn, split, m, n, sums, k):
    """S after the first k coarse steps of dt = T/coarse: the REPLAY hh_mc_solve of k steps over k·dt"""
    coarse = sums.shape[1]
    mk = _ffi.make_model(sigma=m.sigma, T=m.T * k / coarse)
    c = _ffi.make_config(dyn, EULER, n, k, em_split=split, noise_mode=_ffi.HH_NOISE_REPLAY, seeds=seeds_for(n),
                         replay=np.ascontiguousarray(sums[:, :k]), replay_layout=_ffi.HH_REPLAY_TILE_MAJOR)
    term, res = np.empty(n), _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(mk), C.byref(c), C.byref(res), term.ctypes.data))
    return term


@pytest.mark.parametrize("name", list(MODELS))
def test_coarse_leg_is_the_plain_solve_on_the_summed_increments(hhlib, name):
    dyn, split = MODELS[name]
    m = _ffi.make_model(sigma=0.2) if dyn == LOGN else _ffi.make_model()
    steps, every = 16, 4
    sums = summed_increments(hhlib, dyn, m, N, steps)
    dates = [replay_terminal(hhlib, dyn, split, m, N, sums, k) for k in (2, 4, 6, 8)]  # dt = 1/8 exactly in every one
    coarse = coupled_stats(hhlib, m, config(dyn, N, steps, split), every, 0)[:, N:]
    np.testing.assert_array_equal(coarse[pc.S_T], dates[3])
    mx, mn, sm = dates[0].copy(), dates[0].copy(), dates[0].copy()
    for d in dates[1:]:
        mx, mn, sm = np.maximum(mx, d), np.minimum(mn, d), sm + d
    np.testing.assert_array_equal(coarse[pc.MAX_S], mx)
    np.testing.assert_array_equal(coarse[pc.MIN_S], mn)
    np.testing.assert_array_equal(coarse[pc.SUM_S], sm)
    # each log(exp(x)) is off by a few 1e-16 and there are four terms
    worst = float(np.max(np.abs(coarse[pc.SUM_X] - sum(np.log(d) for d in dates))))
    print(f"\n{name}: SUM_X of the coarse leg against the sum of logs: worst {worst:.3g}")
    assert worst <= 1e-13
    # the smallest shape: one coarse step over T
    one = replay_terminal(hhlib, dyn, split, m, N, summed_increments(hhlib, dyn, m, N, 2), 1)
    np.testing.assert_array_equal(coupled_stats(hhlib, m, config(dyn, N, 2, split), 2, 0)[pc.S_T, N:], one)


# ---- (3) lognormal: the coupling is exact up to rounding ---------------------------------------------------------------------

def test_lognormal_legs_agree_up_to_rounding(hhlib):
    """the log-Euler step is exact in law: both legs compute the same sum in a different association — 16 steps of at most
    a few ulp each"""
    m = _ffi.make_model(sigma=0.2)
    for steps, every in SHAPES:
        for start in (0, 1):
            st = coupled_stats(hhlib, m, config(LOGN, N, steps), every, start)
            worst = float(np.max(np.abs(st[pc.S_T, :N] - st[pc.S_T, N:]) / st[pc.S_T, :N]))
            print(f"\nlognormal {steps} steps: fine against coarse S_T, worst relative {worst:.3g}")
            assert worst <= 1e-12


# ---- (4) the payoff differences ---------------------------------------------------------------------------------------------

def test_payoff_differences(hhlib):
    steps, every, start = 16, 4, 1
    m, c = _ffi.make_model(), config(HEST, N, steps)
    payoffs = every_kind(plain_stats(hhlib, m, c, every, start))
    diff, fine, values, stats = coupled_solve(hhlib, m, c, every, start, payoffs)
    np.testing.assert_array_equal(stats, coupled_stats(hhlib, m, c, every, start))
    assert (stats[pc.MAX_S, :N] == payoffs[3].barrier).sum() >= 1
    nm = pc.n_mon(steps, every, start)
    for k, q in enumerate(payoffs):
        for leg, cols in (("fine", slice(0, N)), ("coarse", slice(N, 2 * N))):
            want = bc.payoff_from_stats(stats[:, cols], q, nm, bc.MONITORED)
            if q.kind == pc.GEOM:  # the two exponentials' bounds, as tests/test_gpu_path_payoff.py holds hh_mc_solve_path
                bar = 2.0 * np.spacing(np.exp(stats[pc.SUM_X, cols] / float(nm)))
                assert float(np.max(np.abs(values[k, cols] - want) / bar)) <= 1.0, leg
            else:
                np.testing.assert_array_equal(values[k, cols], want, err_msg=f"payoff {k} kind {q.kind} {leg}")
        y = values[k, :N] - values[k, N:]
        s, ss = math.fsum(y), math.fsum(y * y)
        print(f"\nkind {q.kind}: ΣY off by {abs(diff[k].sum_payoff - s):.3g} (bar {1e-12 * math.fsum(np.abs(y)):.3g}), "
              f"ΣY² by {abs(diff[k].sumsq_payoff - ss):.3g} (bar {1e-12 * ss:.3g})")
        assert abs(diff[k].sum_payoff - s) <= 1e-12 * math.fsum(np.abs(y)), k
        assert abs(diff[k].sumsq_payoff - ss) <= 1e-12 * ss, k
        assert diff[k].price == m.discount * (diff[k].sum_payoff / N) and diff[k].n_paths_done == N
    # a payoff's result does not depend on what else is in the call: five payoffs cross one group of four
    for k in range(5):
        d1, f1, v1, _ = coupled_solve(hhlib, m, c, every, start, [payoffs[k]])
        assert same_result(d1[0], diff[k]) and same_result(f1[0], fine[k]), k
        np.testing.assert_array_equal(v1[0], values[k])
    d5, f5, v5, _ = coupled_solve(hhlib, m, c, every, start, payoffs[:5])
    for k in range(5):
        assert same_result(d5[k], diff[k]) and same_result(f5[k], fine[k]), k
    np.testing.assert_array_equal(v5, values[:5])


# ---- (5) the refusals ------------------------------------------------------------------------------------------------------

def error_rows():
    r = []
    one = lambda **kw: [pc.payoff(**{**dict(kind=pc.ARITH), **kw})]  # noqa: E731

    def add(i, code, text, cfg=None, steps=4, every=2, payoffs=None, n_payoffs=None, null=None, stats_only=False):
        r.append(dict(id=i, code=code, text=text, cfg=cfg or {}, steps=steps, every=every, payoffs=payoffs, n_payoffs=n_payoffs,
                      null=null, stats_only=stats_only))

    who = "hh_mc_solve_path_coupled"
    even = ": n_steps ({}, the fine grid) and monitor_every ({}) must be even: the coarse grid has half the steps and the same dates"
    for null in ("model", "cfg", "payoffs", "out"):
        add("null." + null, INV, who + ": NULL argument", null=null)
    add("steps.odd", INV, who + even.format(3, 1), steps=3, every=1)
    add("every.odd", INV, who + even.format(6, 3), steps=6, every=3)
    add("every.zero", INV, who + ": monitor_every (0) must be >= 1 and divide n_steps (4)", every=0)
    add("every.divisor", INV, who + ": monitor_every (6) must be >= 1 and divide n_steps (8)", steps=8, every=6)
    add("antithetic", UNS, who + ": no antithetic pairs (the second column of a trajectory is its coarse partner)", cfg=dict(antithetic=1))
    add("replay", UNS, who + ": GENERATE noise, no dual partials", cfg=dict(noise_mode=_ffi.HH_NOISE_REPLAY))
    add("partials", UNS, who + ": GENERATE noise, no dual partials", cfg=dict(n_partials=1))
    needs = " needs LognormalDynamics or HestonDynamics + EulerMaruyama"
    add("exact_law", UNS, who + needs, cfg=dict(dyn=LOGN, strat=_ffi.HH_EXACT_LAW))
    add("broadie_kaya", UNS, who + needs, cfg=dict(strat=_ffi.HH_BROADIE_KAYA))
    add("qe", UNS, who + needs, cfg=dict(strat=_ffi.HH_QE))
    add("dynamics", UNS, who + needs, cfg=dict(dyn=7))
    add("n_payoffs.zero", INV, who + ": 1 .. 1024 payoffs", n_payoffs=0)
    add("n_payoffs.max", INV, who + ": 1 .. 1024 payoffs", n_payoffs=1025)
    add("kind", INV, who + ": payoff 0: unknown kind 8", payoffs=one(kind=8))
    add("barrier_type", INV, who + ": payoff 0: unknown barrier type 4", payoffs=one(kind=pc.BARRIER, barrier_type=4, barrier=1.0))
    add("cp", INV, who + ": payoff 0: cp must be +1 or -1", payoffs=one(cp=0.5))
    add("strike.nan", INV, who + ": payoff 0: strike, rebate, cash finite; barrier not NaN", payoffs=one(strike=math.nan))
    who = "hh_mc_path_stats_coupled"
    add("stats.null", INV, who + ": NULL argument", null="stats", stats_only=True)
    add("stats.steps.odd", INV, who + even.format(5, 1), steps=5, every=1, stats_only=True)
    add("stats.every.odd", INV, who + even.format(4, 1), every=1, stats_only=True)
    add("stats.antithetic", UNS, who + ": no antithetic pairs (the second column of a trajectory is its coarse partner)",
        cfg=dict(antithetic=1), stats_only=True)
    add("stats.replay", UNS, who + ": GENERATE noise, no dual partials", cfg=dict(noise_mode=_ffi.HH_NOISE_REPLAY), stats_only=True)
    return r


def test_refusals_leave_the_context_usable():
    ctx = _ffi.Context(0)
    try:
        n = 10
        seeds = seeds_for(n)
        host = np.zeros(2 * ROWS * n)
        out = (_ffi.hh_result * 2)()
        good = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.ARITH))
        m = _ffi.make_model()
        for row in error_rows():
            kw = dict(row["cfg"])
            c = _ffi.make_config(kw.pop("dyn", HEST), kw.pop("strat", EULER), n, row["steps"], seeds=seeds, **kw)
            if c.noise_mode == _ffi.HH_NOISE_REPLAY:
                c.replay, c.replay_len = host.ctypes.data, host.size
            null = row["null"]
            pm, pcfg = (None if null == "model" else C.byref(m)), (None if null == "cfg" else C.byref(c))
            if row["stats_only"]:
                rc = ctx.lib.hh_mc_path_stats_coupled(ctx.handle, pm, pcfg, row["every"], 0,
                                                      None if null == "stats" else host.ctypes.data, 0, None)
            else:
                ps = row["payoffs"]
                arr = (_ffi.hh_path_payoff * len(ps))(*ps) if ps else good
                k = row["n_payoffs"] if row["n_payoffs"] is not None else len(arr)
                rc = ctx.lib.hh_mc_solve_path_coupled(ctx.handle, pm, pcfg, row["every"], 0, None if null == "payoffs" else arr, k,
                                                      None if null == "out" else out, None, None, None)
            assert rc == row["code"], (row["id"], rc, ctx.lib.hh_last_error(ctx.handle).decode())
            assert ctx.lib.hh_last_error(ctx.handle).decode() == row["text"], row["id"]
        # one valid call afterwards still succeeds (out_fine is nullable)
        c = _ffi.make_config(HEST, EULER, n, 4, seeds=seeds)
        ctx.check(ctx.lib.hh_mc_solve_path_coupled(ctx.handle, C.byref(m), C.byref(c), 2, 0, good, 1, out, None, None, None))
        assert out[0].n_paths_done == n and out[0].sumsq_payoff > 0.0
    finally:
        ctx.close()


# ---- (6), (7): the telescoping sum and what the coupling is worth ----------------------------------------------------------------

REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)  # T = 1


def mild_market():
    p = mc.MILD
    return hh.HestonInputs(REF, p["r"], p["S0"], p["V0"], p["kappa"], p["theta"], p["sigma"], p["rho"])


def mild_payoffs(every):
    """the call, the arithmetic Asian call on the 4 dates (every: steps per date), the cash digital"""
    K = mc.MILD["K"]
    return {"call": hh.VanillaOption(K, EXP, hh.European(), hh.Call(), hh.Spot()),
            "asian": hh.AsianOption(K, EXP, hh.Call(), hh.ArithmeticAverage(), hh.Monitoring(every)),
            "digital": hh.DigitalOption(K, EXP, hh.Call(), hh.CashOrNothing(10.0))}


@pytest.fixture(scope="module")
def fixed_solutions():
    """the fixed form on steps 4 → 32, one solve per payoff, shared by (6) and (7)"""
    method = hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.MLMCConfig(mc.STEPS0, trajectories=mc.TRAJECTORIES, seed=7))
    return {name: hh.solve(hh.PricingProblem(p, mild_market()), method) for name, p in mild_payoffs(1).items()}


def test_telescoping_sum_is_the_single_level_price(fixed_solutions):
    """E[P_0] + Σ E[P_l − P_{l−1}] = E[P_L] exactly: the two estimates differ by their standard errors alone"""
    finest = mc.STEPS0 << (len(mc.TRAJECTORIES) - 1)
    single = hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                           hh.SimulationConfig(2 ** 18, steps=finest, seeds=np.random.default_rng(99).integers(0, 2**64, 2 ** 18, dtype=np.uint64)))
    for name, p in mild_payoffs(finest // mc.DATES).items():
        ml, sl = fixed_solutions[name], hh.solve(hh.PricingProblem(p, mild_market()), single, ensemble=False)
        bar = 4.0 * math.sqrt(ml.std_error ** 2 + sl.std_error ** 2)
        print(f"\n{name}: multilevel {ml.price:.5f} ± {ml.std_error:.5f}, single level {sl.price:.5f} ± {sl.std_error:.5f}, "
              f"difference {abs(ml.price - sl.price) / bar * 4.0:.2f} combined standard errors")
        assert ml.converged and [lv.steps for lv in ml.levels] == [4, 8, 16, 32]
        assert [lv.trajectories for lv in ml.levels] == list(mc.TRAJECTORIES)
        assert abs(ml.price - sl.price) <= bar, name


def test_coupling_reduces_the_variance(fixed_solutions):
    for name in ("call", "asian"):
        V = [lv.variance for lv in fixed_solutions[name].levels]
        print(f"\n{name}: Var P_0 = {V[0]:.4g}, V_1 … V_3 = {V[1]:.4g}, {V[2]:.4g}, {V[3]:.4g}; V_1/Var P_0 = {V[1] / V[0]:.4f}, "
              f"V_2/V_1 = {V[2] / V[1]:.3f}, V_3/V_2 = {V[3] / V[2]:.3f}")
        assert V[1] <= mc.V1_OVER_VAR0 * V[0], name
        for l in (1, 2):
            assert V[l + 1] <= mc.DECAY * V[l], (name, l)


# ---- (8) the adaptive form -------------------------------------------------------------------------------------------------------

def test_adaptive_form():
    eps = 0.05
    prob = hh.PricingProblem(mild_payoffs(1)["call"], mild_market())
    method = hh.MultilevelMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.MLMCConfig(mc.STEPS0, tolerance=eps, seed=11))
    sol = hh.solve(prob, method)
    exact = hh.solve(prob, hh.CarrMadan(1.0, 32.0, hh.HestonDynamics())).price
    print(f"\nadaptive: {sol.price:.5f} ± {sol.std_error:.5f} on {[(lv.steps, lv.trajectories) for lv in sol.levels]}, "
          f"bias estimate {sol.bias_estimate:.4f}, Carr–Madan {exact:.5f}, cost {sol.cost:.4g} steps")
    assert sol.converged
    assert sol.std_error <= eps / math.sqrt(2.0) * 1.1  # the 10 %: V_l is estimated from the trajectories themselves
    assert sol.bias_estimate <= eps / math.sqrt(2.0)
    assert abs(sol.price - exact) <= 4.0 * sol.std_error + sol.bias_estimate
    again = hh.solve(prob, method)
    assert again.price == sol.price and again.std_error == sol.std_error and again.levels == sol.levels
