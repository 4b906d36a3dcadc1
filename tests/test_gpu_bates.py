"""Bates — Heston QE paths with Merton jumps — on the device (hh_bates.hip, hh_fourier.hip): hh_mc_path_stats_bates,
hh_mc_solve_path_bates, hh_carr_madan_bates and the Python routes above them.

  * PATH BY PATH against the restatement of tests/bates_cases.py at 50 digits on the draws the device makes itself (the
    oracle's host Philox; the normals restated by hh_rng.h's formulas): the five rows and var_T of every member within
    euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A).  257 trajectories (two workgroups, a one-lane tail), four
    shapes — 5 steps leave the block of jump uniforms half read —, λ·dt = 0.9 so that N takes 0 … 5 within a case.
  * IDENTITIES, bit for bit: λ = 0 is hh_mc_solve_path_qe in every output; hh_carr_madan_bates at λ = 0 is
    hh_carr_madan_basket; a payoff of a Carr–Madan basket prices as it does alone.  SHARED DRAWS: the per-trajectory jump
    totals are those of hh_mc_solve_path_jump on the same seeds.
  * THE LAW, fixed seeds, 2¹⁸ trajectories: calls within 4 standard errors of hh_carr_madan_bates; the mean of S_T under
    the correction; without jumps in the paths the price is more than 10 standard errors away; antithetic pairs.
  * Errors: every HH_ERR_INVALID / HH_ERR_UNSUPPORTED case of the header, with its text, without a launch.
The module prints its worst error/bar per row at its end (`-s`)."""
import ctypes as C
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import bates_cases as bt  # noqa: E402
from tests import carr_madan_cases as cmc  # noqa: E402
from tests import carr_madan_law_cases as cl  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import merton_cases as mc  # noqa: E402
from tests import path_payoff_cases as pc  # noqa: E402
from tests import qe_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

DOC = bt.load_golden()
ROW_NAMES = ("SUM_S", "SUM_X", "MAX_S", "MIN_S", "S_T", "var_T")
_cache = {}


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("Bates (device)")
    yield w
    w.report()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def path_stats(ctx, m, q, j, c, every, start, want_var=True):
    stats, var = np.empty((_ffi.HH_PATH_STATS, n_total(c))), (np.empty(n_total(c)) if want_var else None)
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_bates(ctx.handle, C.byref(m), C.byref(q), C.byref(j), C.byref(c), every, start,
                                             stats.ctypes.data, 0, var.ctypes.data if want_var else None, C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return stats, var


def solve_path(ctx, m, q, j, c, every, start, payoffs, want=True, want_var=False):
    """j None: hh_mc_solve_path_qe"""
    K = len(payoffs)
    arr = (_ffi.hh_path_payoff * K)(*payoffs)
    res = (_ffi.hh_result * K)()
    values, stats = (np.empty((K, n_total(c))), np.empty((_ffi.HH_PATH_STATS, n_total(c)))) if want else (None, None)
    var = np.empty(n_total(c)) if want_var else None
    tail = (arr, K, res, values.ctypes.data if want else None, stats.ctypes.data if want else None,
            var.ctypes.data if want_var else None)
    if j is None:
        ctx.check(ctx.lib.hh_mc_solve_path_qe(ctx.handle, C.byref(m), C.byref(q), C.byref(c), every, start, *tail))
    else:
        ctx.check(ctx.lib.hh_mc_solve_path_bates(ctx.handle, C.byref(m), C.byref(q), C.byref(j), C.byref(c), every, start, *tail))
    return list(res), values, stats, var


RESULT_FIELDS = [f for f, _ in _ffi.hh_result._fields_ if f not in ("kernel_ms", "total_ms", "dprice")]


def same_result(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in RESULT_FIELDS) and list(a.dprice) == list(b.dprice)


def law_seeds(n, salt=3):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt)


# ---- (a) path by path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("include_start", [0, 1])
@pytest.mark.parametrize("shape", bt.PATH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(bt.MODELS))
def test_path_by_path(hhlib, oracle, worst, name, shape, include_start, anti, mart):
    n_steps, every = shape
    case, seeds = bt.path_case(name, n_steps), bt.path_seeds()
    rec = next(b for b in DOC["seen"] if b["model"] == name and b["n_steps"] == n_steps)
    if n_steps > 1:
        assert rec["quadratic"] > 0 and rec["exponential"] > 0 and max(map(int, rec["N"])) >= 2
    d = cached(("d", n_steps), lambda: bt.draws(oracle, seeds, n_steps))
    N = cached(("N", name, n_steps), lambda: bt.counts(d["UJ"], bt.path_mean(case, n_steps)))
    runs = cached(("runs", name, n_steps, mart), lambda: bt.walks(case, n_steps, d, N, 1, mart)[0])
    ref = bt.reference(case, runs[:2 if anti else 1], every, include_start)
    bars = etc.path_bar(ref["e64"], ref["A"])
    stats, var = path_stats(hhlib, bt.model_of(case), _ffi.make_qe(0.0, mart), bt.jump_struct(case),
                            bt.config_of(bt.PATH_N, n_steps, seeds, anti), every, include_start)
    got = np.vstack([stats, var[None, :]])
    bad = []
    for mem in range(ref["members"]):
        for i in range(bt.PATH_N):
            for row in range(6):
                bad.append(worst.check(ROW_NAMES[row], got[row][mem * bt.PATH_N + i], ref["want"][mem][i][row],
                                       bars[mem][i][row], f"{name} {n_steps}x{every} start={include_start} anti={anti} "
                                       f"mart={mart} member {mem} path {i}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ---- (b) identities ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mart", [0, 1])
@pytest.mark.parametrize("anti", [0, 1])
def test_without_jumps_every_output_is_the_qe_solve(hhlib, anti, mart):
    """λ = 0 (μ_J, σ_J set): stats, var_T, path_values and every field of hh_result but the two timings are
    hh_mc_solve_path_qe's, bit for bit — three shapes, 1, 255, 256 and 257 trajectories"""
    case = qc.MODELS["low_v0"]
    m, q, j = qc.model_of(case), _ffi.make_qe(0.0, mart), _ffi.make_jump(0.0, -0.1, 0.15)
    for n_steps, every, start in ((1, 1, 0), (5, 1, 1), (6, 3, 0)):
        for n in (1, 255, 256, 257):
            c = qc.config_of(n, n_steps, law_seeds(n, 31), anti)
            pay = mc.payoff_list()
            a = solve_path(hhlib, m, q, j, c, every, start, pay, want_var=True)
            b = solve_path(hhlib, m, q, None, c, every, start, pay, want_var=True)
            for k in range(len(pay)):
                assert same_result(a[0][k], b[0][k]), (n_steps, n, k)
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y), (n_steps, n)
            assert np.all(np.isfinite(a[2]))


def test_jumps_are_those_of_the_merton_path_form(hhlib):
    """κ = θ = V0 = 1, σ = 1e-3, ρ = 0 against hh_mc_solve_path_jump with σ = √θ on the same seeds, λ, μ_J, σ_J and steps:
    the per-trajectory jump totals — final log spot minus that of the same entry point's λ = 0 solve — agree to 1e-9
    (the same N_k and z at every step; both totals carry the same −λκ̄·T), and they are no zeros"""
    n, n_steps = 257, 6
    seeds = bt.path_seeds()
    jump = dict(lam=0.9 * n_steps, mu_j=-0.1, sigma_j=0.15)
    bcase = dict(S0=100.0, V0=1.0, kappa=1.0, theta=1.0, sigma=1e-3, rho=0.0, r_drift=0.02, T=1.0)
    mcase = dict(S0=100.0, sigma=1.0, r_drift=0.02, T=1.0)
    pay = [pc.payoff(pc.VANILLA, 100.0, 1.0)]

    def bates_x(lam, anti):
        c = qc.config_of(n, n_steps, seeds, anti)
        _, _, st, _ = solve_path(hhlib, qc.model_of(bcase), _ffi.make_qe(0.0, 0), _ffi.make_jump(lam, jump["mu_j"], jump["sigma_j"]),
                                 c, n_steps, 0, pay)
        return st[pc.SUM_X]

    def merton_x(lam, anti):
        c = _ffi.make_config(mc.GBM, mc.EULER, n, n_steps, antithetic=anti, seeds=seeds)
        arr, res = (_ffi.hh_path_payoff * 1)(*pay), (_ffi.hh_result * 1)()
        st = np.empty((_ffi.HH_PATH_STATS, n * (2 if anti else 1)))
        j = _ffi.make_jump(lam, jump["mu_j"], jump["sigma_j"])
        hhlib.check(hhlib.lib.hh_mc_solve_path_jump(hhlib.handle, C.byref(mc.model_of(mcase)), C.byref(j), C.byref(c), n_steps, 0,
                                                    arr, 1, res, None, st.ctypes.data))
        return st[pc.SUM_X]

    for anti in (0, 1):
        tb = bates_x(jump["lam"], anti) - bates_x(0.0, anti)
        tm = merton_x(jump["lam"], anti) - merton_x(0.0, anti)
        worst_gap = float(np.max(np.abs(tb - tm)))
        print(f"\nanti={anti}: largest |Bates − Merton| jump total {worst_gap:.3g}; totals span [{tm.min():.3f}, {tm.max():.3f}]")
        assert worst_gap <= 1e-9
        assert np.ptp(tm) > 0.5 and np.count_nonzero(np.abs(tm - tm[0]) > 1e-3) > n // 2


# ---- (c) the law ---------------------------------------------------------------------------------------------------------------

N_LAW = 2 ** 18
STRIKES = [70.0, 100.0, 140.0]


def carr_madan_bates(ctx, case, strikes, cps=None, Ts=None):
    """hh_carr_madan_bates on the case, α and bound of tests/carr_madan_cases.py's Feller-violating Heston case"""
    _, ref = cmc.BY_ID["feller_violated"]
    K = np.array(strikes, dtype=np.float64)
    n = len(K)
    Ts = np.full(n, case["T"]) if Ts is None else np.array(Ts, dtype=np.float64)
    D = np.exp(-case["r_drift"] * Ts)
    arrs = [K, np.ones(n) if cps is None else np.array(cps, dtype=np.float64), Ts, np.full(n, case["r_drift"]), D]
    out = np.empty(n)
    ctx.check(ctx.lib.hh_carr_madan_bates(ctx.handle, C.byref(qc.model_of(case)), C.byref(bt.jump_struct(case)), ref["alpha"],
                                          ref["bound"], *[a.ctypes.data for a in arrs], n, out.ctypes.data))
    return out


def test_the_law_against_carr_madan(hhlib):
    """κ = 0.3, θ = v₀ = 0.04, σ = 0.9, ρ = −0.5, T = 5 on 16 steps, λ = 0.8, μ_J = −0.1, σ_J = 0.15, expiry-only.  Calls
    at K = 70, 100, 140 within 4 standard errors of hh_carr_madan_bates (an independent Fourier price on the CPU gave
    35.826, 17.507, 5.400; over 8 × 2¹⁸ trajectories of a numpy restatement the mean miss was +0.11 … +0.25 standard
    errors, the largest single one 1.7); with the correction the mean of S_T within 4 standard errors of S0·e^{rT};
    the same solve with λ = 0 in the paths only more than 10 standard errors from the Bates price at K = 100;
    antithetic pairs: a smaller standard error and a price within 4 plain standard errors."""
    case = bt.LAW
    want = carr_madan_bates(hhlib, case, STRIKES)
    np.testing.assert_allclose(want, [35.826, 17.507, 5.400], atol=2e-3)
    seeds = law_seeds(N_LAW)
    m, j = qc.model_of(dict(case, discount=math.exp(-case["r_drift"] * case["T"]))), bt.jump_struct(case)
    payoffs = [pc.payoff(pc.VANILLA, K, 1.0) for K in STRIKES]
    plain, _, _, _ = solve_path(hhlib, m, _ffi.make_qe(0.0, 0), j, qc.config_of(N_LAW, 16, seeds), 16, 0, payoffs, want=False)
    for r, w, K in zip(plain, want, STRIKES):
        miss = (r.price - w) / r.std_error
        print(f"\nBates K={K:g}: price {r.price:.5f}, Carr–Madan {w:.5f}, {miss:+.2f} standard errors of {r.std_error:.4f}")
        assert r.std_error > 0.0 and abs(miss) <= 4.0, (K, r.price, w, r.std_error)
    _, _, stats, _ = solve_path(hhlib, m, _ffi.make_qe(0.0, 1), j, qc.config_of(N_LAW, 16, seeds), 16, 0, payoffs[:1])
    S = stats[pc.S_T]
    fwd = case["S0"] * math.exp(case["r_drift"] * case["T"])
    miss = (S.mean() - fwd) / (S.std(ddof=1) / math.sqrt(N_LAW))
    print(f"\ncorrected: mean S_T {S.mean():.4f}, {miss:+.2f} standard errors from {fwd:.4f}")
    assert abs(miss) <= 4.0
    none, _, _, _ = solve_path(hhlib, m, _ffi.make_qe(0.0, 0), _ffi.make_jump(0.0, case["mu_j"], case["sigma_j"]),
                               qc.config_of(N_LAW, 16, seeds), 16, 0, payoffs[1:2], want=False)
    miss = (none[0].price - want[1]) / none[0].std_error
    print(f"\nno jumps in the paths, K=100: price {none[0].price:.5f}, {miss:+.2f} standard errors")
    assert abs(miss) > 10.0
    anti, _, _, _ = solve_path(hhlib, m, _ffi.make_qe(0.0, 0), j, qc.config_of(N_LAW, 16, seeds, 1), 16, 0, payoffs[1:2], want=False)
    print(f"\nK=100 standard error plain {plain[1].std_error:.5f}, antithetic {anti[0].std_error:.5f}")
    assert 0.0 < anti[0].std_error < plain[1].std_error
    assert abs(anti[0].price - want[1]) <= 4.0 * plain[1].std_error


# ---- (d) Carr–Madan on the device ----------------------------------------------------------------------------------------------

def cm_call(ctx, entry, case, payoffs, jump=True):
    """payoffs: (K, cp, T) rows under the case's model, rate, α and bound -> prices by hh_carr_madan_bates / _basket"""
    K, cp, Ts = (np.array([p[i] for p in payoffs], dtype=np.float64) for i in range(3))
    n = len(K)
    arrs = [K, cp, Ts, np.full(n, case["r_drift"]), np.array([math.exp(-case["r_drift"] * T) for T in Ts])]
    out, m = np.empty(n), qc.model_of(case)
    ptrs = [a.ctypes.data for a in arrs]
    if jump:
        ctx.check(ctx.lib.hh_carr_madan_bates(ctx.handle, C.byref(m), C.byref(bt.jump_struct(case)), case["alpha"], case["bound"],
                                              *ptrs, n, out.ctypes.data))
    else:
        ctx.check(ctx.lib.hh_carr_madan_basket(ctx.handle, C.byref(m), _ffi.HH_HESTON, 0, case["alpha"], case["bound"], *ptrs, n,
                                               out.ctypes.data))
    return out


@pytest.mark.parametrize("key", list(bt.CM_CASES))
def test_carr_madan_against_the_exact_integral(hhlib, worst, key):
    """every case of the fixture against its exactly integrated truncated integral, inside merton_cases.cm_bar; the put
    through the parity transform; λ = 0 bit-equal to hh_carr_madan_basket"""
    case, rec = bt.cm_cases()[key], DOC["carr_madan"][key]
    assert case["discount"] == math.exp(-case["r_drift"] * case["T"])
    got = cm_call(hhlib, None, case, [(case["K"], case["cp"], case["T"])])[0]
    with mp.workdps(qc.DPS):
        want = mp.mpf(rec["call"]) + (cl.cm_parity(case) if case["cp"] < 0 else 0)
        assert not worst.check("carr-madan", got, want, bt.cm_bar(case["S0"], rec["e64"]), key)
    if case["cp"] < 0:
        call = cm_call(hhlib, None, case, [(case["K"], 1.0, case["T"])])[0]
        assert got == call - case["S0"] + case["K"] * case["discount"]
    if case["lam"] == 0.0:
        assert got == cm_call(hhlib, None, case, [(case["K"], case["cp"], case["T"])], jump=False)[0]


def test_carr_madan_baskets_price_each_payoff_as_alone(hhlib):
    """baskets of 1, 2 and 257 payoffs — calls and puts, two expiries: every payoff to the bits it has alone; at λ = 0
    the whole basket is hh_carr_madan_basket's, bit for bit"""
    case = bt.cm_cases()["feller_violated"]
    rows = [(60.0 + 0.35 * k, 1.0 if k % 3 else -1.0, 2.0 if k % 2 else 0.75) for k in range(257)]
    big = cm_call(hhlib, None, case, rows)
    assert np.all(np.isfinite(big)) and np.all(big > 0.0)
    assert cm_call(hhlib, None, case, rows[:1])[0] == big[0]
    assert np.array_equal(cm_call(hhlib, None, case, rows[:2]), big[:2])
    for k in (1, 17, 128, 255, 256):
        assert cm_call(hhlib, None, case, [rows[k]])[0] == big[k], k
    quiet = dict(case, lam=0.0)
    assert np.array_equal(cm_call(hhlib, None, quiet, rows), cm_call(hhlib, None, quiet, rows, jump=False))


# ---- (e) errors ------------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
BAD_JUMPS = [  # (λ, μ_J, σ_J), text
    ((-1.0, 0.0, 0.1), "jump lambda must be finite and >= 0"), ((NAN, 0.0, 0.1), "jump lambda must be finite and >= 0"),
    ((INF, 0.0, 0.1), "jump lambda must be finite and >= 0"), ((1.0, 0.0, -0.1), "jump sigma_j must be finite and >= 0"),
    ((1.0, 0.0, NAN), "jump sigma_j must be finite and >= 0"), ((1.0, 0.0, INF), "jump sigma_j must be finite and >= 0"),
    ((1.0, NAN, 0.1), "jump mu_j must be finite"), ((1.0, INF, 0.1), "jump mu_j must be finite"),
    ((1.0, -INF, 0.1), "jump mu_j must be finite"), ((1.0, 800.0, 0.1), "exp(mu_j + sigma_j^2/2) must be finite"),
]


def test_errors_come_back_without_a_launch(hhlib):
    """every HH_ERR_INVALID and HH_ERR_UNSUPPORTED case of the header, hostile scalars included, with its text and the
    entry point's name; no timing slot is opened (nothing was launched) and the context solves afterwards.  The
    existing entry points still refuse HH_QE with hh_jump, and Heston with hh_mc_solve_path_jump."""
    ctx = hhlib
    case = bt.path_case("feller", 4)
    n, steps = 300, 4
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    good_m, good_q, good_j = qc.model_of(case), _ffi.make_qe(0.0, 0), bt.jump_struct(case)
    outs = (_ffi.hh_result * 1)()
    pay = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.VANILLA, 100.0, 1.0))
    stats = np.empty((5, n))
    cfg = lambda **kw: qc.config_of(n, steps, seeds, **kw)  # noqa: E731
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731

    def both(mm, qq, jj, cc, every=1, arr=pay, k=1):
        a = ctx.lib.hh_mc_solve_path_bates(ctx.handle, ref(mm), ref(qq), ref(jj), ref(cc), every, 0, arr, k, outs, None, None, None)
        ta = ctx.lib.hh_last_error(ctx.handle).decode()
        b = ctx.lib.hh_mc_path_stats_bates(ctx.handle, ref(mm), ref(qq), ref(jj), ref(cc), every, 0, stats.ctypes.data, 0, None, None)
        return (a, ta), (b, ctx.lib.hh_last_error(ctx.handle).decode())

    def expect(mm, qq, jj, cc, code, text, **kw):
        for who, (rc, msg) in zip(("hh_mc_solve_path_bates", "hh_mc_path_stats_bates"), both(mm, qq, jj, cc, **kw)):
            assert rc == code and text in msg and who in msg, (who, rc, code, text, msg)

    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
        expect(good_m, None, good_j, cfg(), INV, "NULL argument")
        expect(good_m, good_q, None, cfg(), INV, "NULL argument")
        expect(None, good_q, good_j, cfg(), INV, "NULL argument")
        expect(good_m, good_q, good_j, None, INV, "NULL argument")
        for (lam, mu, sj), text in BAD_JUMPS:
            expect(good_m, good_q, _ffi.make_jump(lam, mu, sj), cfg(), INV, text)
        over = _ffi.make_jump(64.0 * steps / case["T"] * (1 + 1e-12), 0.0, 0.1)  # λ·T/n_steps just above the limit
        expect(good_m, good_q, over, cfg(), INV, "is above HH_JUMP_MAX_MEAN")
        for d in (dict(kappa=0.0), dict(kappa=-1.0), dict(theta=0.0), dict(sigma=0.0), dict(sigma=-0.5), dict(V0=-1e-9)):
            expect(qc.model_of(dict(case, **d)), good_q, good_j, cfg(), INV, "kappa, theta, sigma must be > 0 and V0 >= 0")
        for d in (dict(rho=1.0000001), dict(kappa=NAN), dict(theta=INF), dict(V0=NAN), dict(sigma=NAN), dict(rho=NAN),
                  dict(r_drift=INF), dict(T=INF), dict(S0=-1.0), dict(T=0.0)):
            expect(qc.model_of(dict(case, **d)), good_q, good_j, cfg(), INV, "model scalars finite")
        for psi in (0.5, 0.999999, 2.0000001, -1.0, NAN, INF):
            expect(good_m, _ffi.make_qe(psi, 0), good_j, cfg(), INV, "psi_c must be 0 (the default 1.5) or lie in [1, 2]")
        expect(qc.model_of(dict(case, kappa=1e-20, sigma=1e-8)), good_q, good_j, cfg(), INV, "rounds to 0")
        expect(qc.model_of(dict(case, sigma=100.0, theta=1e-6)), good_q, good_j, cfg(), INV, "is above HH_QE_MAX_PSI")
        # the step's constants are formed on r_c: r = −1.5e308 and λκ̄ = expm1(709) = 8.2e307 are finite, r − λκ̄ is not
        expect(qc.model_of(dict(case, r_drift=-1.5e308, discount=1.0)), good_q, _ffi.make_jump(1.0, 709.0, 0.0), cfg(), INV, "constants are not finite")
        expect(good_m, good_q, good_j, cfg(), INV, "must be >= 1 and divide n_steps", every=3)
        expect(good_m, good_q, good_j, qc.config_of(0, steps, seeds), INV, "1 <= n_paths")
        rc = ctx.lib.hh_mc_solve_path_bates(ctx.handle, C.byref(good_m), C.byref(good_q), C.byref(good_j), C.byref(cfg()), 1, 0,
                                            (_ffi.hh_path_payoff * 1)(pc.payoff(8, 100.0, 1.0)), 1, outs, None, None, None)
        assert rc == INV and "hh_mc_solve_path_bates: payoff 0: unknown kind 8" in ctx.lib.hh_last_error(ctx.handle).decode()
        rc = ctx.lib.hh_mc_solve_path_bates(ctx.handle, C.byref(good_m), C.byref(good_q), C.byref(good_j), C.byref(cfg()), 1, 0, pay,
                                            0, outs, None, None, None)
        assert rc == INV and "payoffs" in ctx.lib.hh_last_error(ctx.handle).decode()
        # unsupported
        for dyn, strat in ((_ffi.HH_LOGNORMAL, _ffi.HH_QE), (_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA),
                           (_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA), (_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA)):
            expect(good_m, good_q, good_j, _ffi.make_config(dyn, strat, n, steps, seeds=seeds), UNS,
                   "needs HestonDynamics + the quadratic-exponential strategy (HH_QE)")
        expect(good_m, good_q, good_j, cfg(noise_mode=_ffi.HH_NOISE_REPLAY, replay=np.zeros(4)), UNS, "GENERATE noise, no dual partials")
        expect(good_m, good_q, good_j, cfg(n_partials=2), UNS, "GENERATE noise, no dual partials")
        expect(qc.model_of(dict(case, rho=0.9)), _ffi.make_qe(0.0, 1), good_j, cfg(), UNS, "run without it")
        # the existing entry points refuse the mixes they refused: HH_QE with hh_jump, Heston with hh_mc_solve_path_jump
        rc = ctx.lib.hh_mc_solve_path_jump(ctx.handle, C.byref(good_m), C.byref(good_j), C.byref(cfg()), 1, 0, pay, 1, outs, None, None)
        assert rc == UNS and "hh_mc_solve_path_jump needs LognormalDynamics + EulerMaruyama" in ctx.lib.hh_last_error(ctx.handle).decode()
        rc = ctx.lib.hh_mc_solve_path_jump(ctx.handle, C.byref(good_m), C.byref(good_j),
                                           C.byref(_ffi.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, n, steps, seeds=seeds)),
                                           1, 0, pay, 1, outs, None, None)
        assert rc == UNS and "hh_mc_solve_path_jump needs LognormalDynamics + EulerMaruyama" in ctx.lib.hh_last_error(ctx.handle).decode()
        res = _ffi.hh_result()
        assert ctx.lib.hh_mc_solve_jump(ctx.handle, C.byref(good_m), C.byref(good_j), C.byref(cfg()), C.byref(res), None) == UNS
        assert ctx.read_timings() == []  # nothing was launched
        # Carr–Madan
        arrs = [np.array([x]) for x in (105.0, 1.0, 1.0, 0.03, math.exp(-0.03))]
        price = np.empty(1)

        def cm(mm, jj, alpha=1.0, bound=32.0, k=1, a=arrs):
            return ctx.lib.hh_carr_madan_bates(ctx.handle, ref(mm), ref(jj), alpha, bound, *[x.ctypes.data for x in a], k, price.ctypes.data)

        def cm_expect(rc, text):
            msg = ctx.lib.hh_last_error(ctx.handle).decode()
            assert rc == INV and "hh_carr_madan_bates: " + text in msg, (rc, text, msg)

        cm_expect(cm(good_m, None), "NULL argument")
        cm_expect(cm(None, good_j), "NULL argument")
        for (lam, mu, sj), text in BAD_JUMPS:
            cm_expect(cm(good_m, _ffi.make_jump(lam, mu, sj)), text)
        cm_expect(cm(good_m, good_j, alpha=0.0), "bad scalars")
        cm_expect(cm(qc.model_of(dict(case, sigma=0.0)), good_j), "bad scalars")
        cm_expect(cm(qc.model_of(dict(case, S0=0.0)), good_j), "bad scalars")
        cm_expect(cm(good_m, good_j, alpha=1e-4), "bound/alpha must be <= 196608")
        cm_expect(cm(good_m, good_j, k=0), "1 .. 2^20 payoffs per call")
        cm_expect(cm(good_m, good_j, a=[np.array([x]) for x in (-105.0, 1.0, 1.0, 0.03, 0.97)]), "payoff 0: strike, T, discount > 0, cp = +-1")
        assert cm(good_m, _ffi.make_jump(500.0, -0.1, 0.15)) == _ffi.HH_OK and math.isfinite(price[0])  # no draw: λ·T = 500 is no limit
        assert cm(good_m, good_j) == _ffi.HH_OK and price[0] > 0.0
        # the context solves; ρ > 0 without the correction and the mean of exactly HH_JUMP_MAX_MEAN are admitted
        edge = _ffi.make_jump(64.0 * steps / case["T"], -0.01, 0.02)
        res, _, st, var = solve_path(ctx, good_m, _ffi.make_qe(2.0, 1), edge, cfg(), 2, 1, [pc.payoff(pc.VANILLA, 100.0, 1.0)], want_var=True)
        assert np.all(np.isfinite(st)) and np.all(var >= 0.0) and res[0].n_paths_done == n
        st, var = path_stats(ctx, qc.model_of(dict(case, rho=0.9, V0=0.0)), good_q, good_j, cfg(anti=1), 1, 0)
        assert np.all(np.isfinite(st)) and np.all(var >= 0.0)
        assert len(ctx.read_timings()) == 3  # two slots for the solve, one for the statistics alone
    finally:
        ctx.enable_timing(False)


# ---- (f) through solve -----------------------------------------------------------------------------------------------------

def test_python_routes_give_the_c_calls_numbers(hhlib):
    """every payoff class on the Bates route equals its row of one hh_mc_solve_path_bates call; a basket prices equal to
    the single solves; CarrMadan(BatesDynamics()) is hh_carr_madan_bates"""
    ref_, exp_ = hh.Date(2021, 1, 1), hh.Date(2024, 1, 1)
    case = bt.LAW
    mkt = hh.BatesInputs(ref_, 0.0, case["S0"], case["V0"], case["kappa"], case["theta"], case["sigma"], case["rho"],
                         case["lam"], case["mu_j"], case["sigma_j"])
    n, steps = 4096, 12
    seeds = law_seeds(n, 23)
    T = hh.yearfrac(ref_, exp_)
    for strat, anti in ((hh.HestonQE(), False), (hh.HestonQE(psi_c=1.2, martingale=True), True)):
        vr = hh.Antithetic() if anti else hh.NoVarianceReduction()
        method = hh.MonteCarlo(hh.BatesDynamics(), strat, hh.SimulationConfig(n, steps=steps, seeds=seeds, variance_reduction=vr))
        mon = hh.Monitoring(3)
        claims = [(hh.VanillaOption(105.0, exp_, hh.European(), hh.Call(), hh.Spot()), pc.payoff(pc.VANILLA, 105.0, 1.0), steps),
                  (hh.AsianOption(100.0, exp_, hh.Call(), monitoring=mon), pc.payoff(pc.ARITH, 100.0, 1.0), 3),
                  (hh.BarrierOption(100.0, 70.0, exp_, hh.Call(), hh.DownAndOut(), monitoring=mon),
                   pc.payoff(pc.BARRIER, 100.0, 1.0, pc.DOWN_OUT, 70.0, 0.0), 3),
                  (hh.DigitalOption(101.0, exp_, hh.Put()), None, steps),
                  (hh.LookbackOption(exp_, hh.Call(), monitoring=mon), None, 3)]
        m = qc.model_of(dict(case, T=T, discount=1.0))
        q, j = _ffi.make_qe(strat.psi_c, strat.martingale), bt.jump_struct(case)
        c = qc.config_of(n, steps, seeds, int(anti))
        from hedgehog_jl_amd.montecarlo import pack_path_payoff
        for payoff, packed, every in claims:
            sol = hh.solve(hh.PricingProblem(payoff, mkt), method)
            row = pack_path_payoff(payoff)
            if packed is not None:
                assert (row.kind, row.strike, row.cp, row.barrier) == (packed.kind, packed.strike, packed.cp, packed.barrier)
            res, _, stats, _ = solve_path(hhlib, m, q, j, c, every, 0, [row])
            assert sol.price == res[0].price and sol.std_error == res[0].std_error and sol.price > 0.0, type(payoff).__name__
            assert np.array_equal(sol.ensemble, stats)
        basket = hh.solve(hh.BasketPricingProblem([p for p, _, _ in claims], mkt), method)
        for (p, _, _), s in zip(claims, basket.solutions):
            assert s.price == hh.solve(hh.PricingProblem(p, mkt), method).price
    _, cref = cmc.BY_ID["feller_violated"]
    cm = hh.CarrMadan(cref["alpha"], cref["bound"], hh.BatesDynamics())
    call, put = claims[0][0], hh.VanillaOption(95.0, exp_, hh.European(), hh.Put(), hh.Spot())
    want = carr_madan_bates(hhlib, dict(case, T=T), [105.0, 95.0], cps=[1.0, -1.0])
    assert hh.solve(hh.PricingProblem(call, mkt), cm).price == want[0]
    cmb = hh.solve(hh.BasketPricingProblem([call, put], mkt), cm)
    assert [s.price for s in cmb.solutions] == list(want)


def test_finite_difference_greeks_agree_with_carr_madan(hhlib):
    """FiniteDifference delta and a bump in jump_intensity on the Monte Carlo route against the same finite difference on
    CarrMadan(BatesDynamics()): the relative bars and the 2¹⁶ trajectories of test_gpu_merton.py's Greeks (the solves of
    a difference share their seeds; a bumped intensity moves whole jumps in and out of a few trajectories)"""
    ref_, exp_ = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)
    mkt = hh.BatesInputs(ref_, 0.03, 100.0, 0.04, 2.0, 0.04, 0.3, -0.7, 0.8, -0.1, 0.15)
    prob = hh.PricingProblem(hh.VanillaOption(105.0, exp_, hh.European(), hh.Call(), hh.Spot()), mkt)
    n = 2 ** 16
    seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    method = hh.MonteCarlo(hh.BatesDynamics(), hh.HestonQE(), hh.SimulationConfig(n, steps=12, seeds=seeds,
                                                                                  variance_reduction=hh.Antithetic()))
    cm = hh.CarrMadan(1.0, 200.0, hh.BatesDynamics())
    for lens, rel in ((hh.SpotLens(), 0.05), (hh.optic("market_inputs.jump_intensity"), 0.3)):
        fd = hh.FiniteDifference(1e-2)
        want = hh.solve(hh.GreekProblem(prob, lens), fd, cm).greek
        got = hh.solve(hh.GreekProblem(prob, lens), fd, method).greek
        print(f"\n{type(lens).__name__}: Monte Carlo {got:.5f}, Carr–Madan {want:.5f}")
        assert got == pytest.approx(want, rel=rel), lens
