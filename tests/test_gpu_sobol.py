"""Quasi-Monte Carlo on the device (include/hedgehog_mc.h, "Quasi-Monte Carlo"; hh_sobol.hip):

(a) hh_sobol_points against the numpy rule of tests/sobol_cases.py, exactly: point counts around the tile, offsets that make a
    tile cross a multiple of 256 (the two high words of a tile) and that end at point 2^32 − 1, unshifted and under two
    randomisations; the shift words against the oracle's host Philox.
(b) hh_sobol_fill path by path against the 50-digit restatement: the mpmath quantile of the exact u, then the bridge in the
    header's operation order; the bar is euler_tangent_cases.path_bar(e64, A) with the magnitudes carried through
    wl·W_l + wr·W_r + sd·z, plus what the quantile's own bar (tests/math_bars.py) moves the number by.  257 points (two
    workgroups, a one-lane tail); the padded lanes are zero.  The 50-digit quantiles of the 252-step shape take a few
    seconds, once: its four cases share them, and the two values of ρ share the steps.
(c) shards compose bit for bit; the incremental form is the quantile of the point's own coordinate, bit for bit.
(d) one randomisation of each supported pair against the CPU oracle run in REPLAY mode on the copied buffer.
(e) convergence on the fixed seeds of tests/sobol_cases.py, and the Greeks.
(f) every HH_ERR_INVALID / HH_ERR_UNSUPPORTED case; the context stays usable after each."""
import ctypes as C
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import hedgehog_jl_amd as hh  # noqa: E402
from hedgehog_jl_amd import _ffi  # noqa: E402
from hedgehog_jl_amd import montecarlo as hmc  # noqa: E402
from tests import sobol_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

GBM, HES = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON
INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
REF, EXP = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1)


def dev_points(ctx, n_dims, n, offset, shifted=0, randomization=0, seed=0):
    buf = _ffi.DeviceBuffer(ctx, 4 * n_dims * n)
    ctx.check(ctx.lib.hh_sobol_points(ctx.handle, n_dims, n, offset, seed, randomization, shifted, buf.ptr))
    ctx.synchronize()
    out = buf.download(np.empty((n_dims, n), dtype=np.uint32))
    buf.free()
    return out


def dev_fill(ctx, dyn, rho, T, n_steps, n, offset, construction, shifted=1, randomization=sc.FILL_RANDOMIZATION,
             seed=sc.FILL_SEED):
    elems = ctx.lib.hh_replay_elems(n, n_steps, dyn)
    buf = _ffi.DeviceBuffer(ctx, 8 * elems)
    # a pattern the fill must overwrite everywhere, the padded lanes included
    buf.upload(np.full(elems, np.nan))
    ctx.check(ctx.lib.hh_sobol_fill(ctx.handle, dyn, rho, T, n_steps, n, offset, seed, randomization, shifted, construction,
                                    buf.ptr))
    ctx.synchronize()
    out = buf.download(np.empty(elems))
    buf.free()
    return out


# ---- (a) the points --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", sc.POINT_OFFSETS)
def test_points_equal_the_numpy_rule(hhlib, offset):
    v = sc.directions(sc.POINT_DIMS)
    for n in sc.POINT_COUNTS:
        idx = np.arange(offset, offset + n, dtype=np.uint64)
        want = sc.points(v, idx)
        for shifted, r in ((0, 0), (1, 0), (1, 5)):
            got = dev_points(hhlib, sc.MAX_DIMS, n, offset, shifted, r, sc.SHIFT_SEED)[list(sc.POINT_DIMS)]
            shift = sc.shift_words(sc.POINT_DIMS, r, sc.SHIFT_SEED)[:, None] if shifted else np.uint32(0)
            np.testing.assert_array_equal(got, want ^ shift, err_msg=f"offset {offset} n {n} shifted {shifted} r {r}")


def test_shift_words_are_the_oracles_philox(hhlib, oracle):
    key = [sc.SHIFT_SEED & 0xFFFFFFFF, sc.SHIFT_SEED >> 32]
    plain = dev_points(hhlib, sc.MAX_DIMS, 1, 0)
    assert not plain.any()  # point 0 is the origin: a shifted point 0 is the shift itself
    for r in (0, 5):
        got = dev_points(hhlib, sc.MAX_DIMS, 1, 0, 1, r, sc.SHIFT_SEED)[:, 0]
        for d in sc.POINT_DIMS + (2, 3, 4, 7):
            assert got[d] == oracle.philox([d >> 2, r, 0, sc.DOM_SOBOL], key)[d & 3], (d, r)
        np.testing.assert_array_equal(got, sc.shift_words(np.arange(sc.MAX_DIMS), r, sc.SHIFT_SEED))


# ---- (b) the fill, path by path ----------------------------------------------------------------------------------------------

_refs = {}


def fill_reference(n_steps, ncomp, construction, rho):
    key = (n_steps, ncomp, construction, rho if ncomp == 2 else 0.0)
    if key not in _refs:
        x = sc.words(np.arange(ncomp * n_steps), np.arange(sc.FILL_POINTS, dtype=np.uint64), True, sc.FILL_RANDOMIZATION,
                     sc.FILL_SEED)
        _refs[key] = sc.fill_reference(n_steps, ncomp, construction, key[3], sc.FILL_T, x)
    return _refs[key]


@pytest.mark.parametrize("rho", sc.FILL_RHOS)
@pytest.mark.parametrize("construction", [sc.INCREMENTAL, sc.BRIDGE])
@pytest.mark.parametrize("n_steps,ncomp", sc.FILL_SHAPES)
def test_fill_matches_the_50_digit_restatement(hhlib, n_steps, ncomp, construction, rho):
    dyn = HES if ncomp == 2 else GBM
    buf = dev_fill(hhlib, dyn, rho, sc.FILL_T, n_steps, sc.FILL_POINTS, 0, construction)
    got, pad = sc.untile(buf, sc.FILL_POINTS, n_steps, ncomp)
    assert pad.shape[0] == 2 * sc.TILE - sc.FILL_POINTS and not pad.any()  # zeros, not the pattern
    assert np.isfinite(got).all()
    hi, lo, bars = fill_reference(n_steps, ncomp, construction, rho)
    err = sc.fill_errors(got, hi, lo)
    print(f"\nfill {n_steps}x{ncomp} construction {construction} rho {rho}: worst error / bar = {(err / bars).max():.3g}")
    bad = np.argwhere(~(err <= bars))
    assert bad.size == 0, [(tuple(i), got[tuple(i)], hi[tuple(i)], err[tuple(i)], bars[tuple(i)]) for i in bad[:10]]


# ---- (c) shards, and the incremental form ------------------------------------------------------------------------------------

@pytest.mark.parametrize("construction", [sc.INCREMENTAL, sc.BRIDGE])
@pytest.mark.parametrize("a", [256, 3])
def test_shards_compose(hhlib, construction, a):
    """a fill of [a, 513) holds the columns of a fill of [0, 513): a = 256 starts on a tile, a = 3 makes every tile of the
    shard cross a multiple of 256"""
    n_steps, b = 8, 513
    whole, _ = sc.untile(dev_fill(hhlib, HES, -0.7, 1.0, n_steps, b, 0, construction), b, n_steps, 2)
    part, pad = sc.untile(dev_fill(hhlib, HES, -0.7, 1.0, n_steps, b - a, a, construction), b - a, n_steps, 2)
    assert not pad.any()
    np.testing.assert_array_equal(part.view(np.uint64), whole[a:].view(np.uint64))


def word_to_first_dimension_point(x):
    """the point whose dimension-0 word (van der Corput: the bit reversal of its Gray code) is x"""
    g = int(f"{int(x):032b}"[::-1], 2)
    i = 0
    while g:
        i ^= g
        g >>= 1
    return i


def test_incremental_is_the_quantile_of_the_points_own_coordinate(hhlib):
    """With HH_SOBOL_INCREMENTAL, dW/sqrt_dt at sqrt_dt = 1/4 is the quantile of coordinate ncomp·step + comp, bit for bit
    (ρ = 0: the second component is fma(0, d1, 1·d2) = d2).  The device's quantile of a word comes from another route:
    dimension 0 is a bijection of the 32-bit words, so a one-step fill of the ONE unshifted point whose first coordinate
    is that word (T = 1: dW = z) evaluates it."""
    n, ctx = sc.FILL_POINTS, hhlib
    idx = np.arange(n, dtype=np.uint64)
    x = sc.words(np.arange(4), idx, True, sc.FILL_RANDOMIZATION, sc.FILL_SEED)
    uniq = sorted({int(w) for w in x.ravel()})
    buf = _ffi.DeviceBuffer(ctx, 8 * sc.TILE * len(uniq))
    for k, w in enumerate(uniq):
        ctx.check(ctx.lib.hh_sobol_fill(ctx.handle, GBM, 0.0, 1.0, 1, 1, word_to_first_dimension_point(w), 0, 0, 0,
                                        sc.INCREMENTAL, buf.ptr + 8 * sc.TILE * k))
    ctx.synchronize()
    q = dict(zip(uniq, buf.download(np.empty((len(uniq), sc.TILE)))[:, 0]))
    buf.free()
    assert all(np.isfinite(t) for t in q.values())
    for dyn, ncomp, n_steps in ((HES, 2, 2), (GBM, 1, 3)):
        got, _ = sc.untile(dev_fill(ctx, dyn, 0.0, n_steps / 16.0, n_steps, n, 0, sc.INCREMENTAL), n, n_steps, ncomp)
        want = np.array([[[q[int(x[ncomp * k + c, p])] for c in range(ncomp)] for k in range(n_steps)] for p in range(n)])
        np.testing.assert_array_equal((got * 4.0).view(np.uint64), want.view(np.uint64))


# ---- (d) parity with the CPU oracle ------------------------------------------------------------------------------------------

def problem(heston, K=100.0, S0=100.0):
    payoff = hh.VanillaOption(K, EXP, hh.European(), hh.Call(), hh.Spot())
    m = sc.HESTON if heston else sc.LOGNORMAL
    mkt = hh.HestonInputs(REF, m["r"], S0, m["V0"], m["kappa"], m["theta"], m["sigma"], m["rho"]) if heston else \
        hh.BlackScholesInputs(REF, m["r"], S0, m["sigma"])
    return hh.PricingProblem(payoff, mkt)


PAIRS = {"exact": (False, hh.LognormalDynamics, hh.BlackScholesExact, 1e-13),
         "gbm-euler": (False, hh.LognormalDynamics, hh.EulerMaruyama, 1e-12),
         "heston-euler": (True, hh.HestonDynamics, hh.EulerMaruyama, 1e-12)}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_one_randomisation_matches_the_cpu_oracle(hhlib, oracle, pair):
    """513 points, 8 steps: the filled buffer copied to the host, the oracle's REPLAY solve on it, against the library's
    estimate of that randomisation — within test_gpu_parity.py's bars for REPLAY solves (1e-12 Euler, 1e-13 exact law)"""
    heston, dyn, strat, rtol = PAIRS[pair]
    n, steps, seed = 513, 8, 77
    method = hh.QuasiMonteCarlo(dyn(), strat(), hh.SobolConfig(n, steps=steps, randomizations=1, seed=seed))
    prob = problem(heston)
    sol = hh.solve(prob, method)
    assert len(sol.estimates) == 1 and sol.price == sol.estimates[0] and math.isnan(sol.std_error)
    model, c, _, P, _ = hmc._model_and_config(prob, method)
    euler = strat is hh.EulerMaruyama
    fdyn, fsteps, fT = (c.dynamics, steps, model.T) if euler else (GBM, 1, 1.0)
    buf = dev_fill(hhlib, fdyn, model.rho, fT, fsteps, n, 0, sc.BRIDGE, 1, 0, seed)
    c.noise_mode, c.replay_layout = _ffi.HH_NOISE_REPLAY, _ffi.HH_REPLAY_TILE_MAJOR
    c.replay, c.replay_len = buf.ctypes.data, buf.size
    ro, _, _ = oracle.mc_solve(model, c, want_terminal=False)
    assert P == 0 and ro.price > 0.0
    assert sol.estimates[0] == pytest.approx(ro.price, rel=rtol, abs=1e-300)


# ---- (e) convergence and Greeks ------------------------------------------------------------------------------------------------

def black_scholes(m):
    d1 = (math.log(m["S0"] / m["K"]) + (m["r"] + 0.5 * m["sigma"] ** 2) * m["T"]) / (m["sigma"] * math.sqrt(m["T"]))
    d2 = d1 - m["sigma"] * math.sqrt(m["T"])
    N = lambda t: 0.5 * (1.0 + math.erf(t / math.sqrt(2.0)))  # noqa: E731
    return m["S0"] * N(d1) - m["K"] * math.exp(-m["r"] * m["T"]) * N(d2), N(d1)


def test_exact_law_converges_to_black_scholes(hhlib):
    T = hh.yearfrac(REF, EXP)
    price, _ = black_scholes(dict(sc.LOGNORMAL, T=T))
    sol = hh.solve(problem(False), hh.QuasiMonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(),
                                                      hh.SobolConfig(sc.CONV_N_EXACT, randomizations=sc.CONV_R, seed=sc.CONV_SEED)))
    print(f"\nexact law: {sol.price:.8f} ± {sol.std_error:.2e}, Black–Scholes {price:.8f}")
    assert len(sol.estimates) == sc.CONV_R and sol.std_error > 0.0
    assert abs(sol.price - price) <= 4.0 * sol.std_error


def pseudo_random(heston_prob, n, steps):
    seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return hh.solve(heston_prob, hh.MonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), hh.SimulationConfig(n, steps=steps, seeds=seeds)),
                    ensemble=False)


def test_heston_bridge_converges_and_beats_pseudo_random(hhlib):
    """(b) within 4 combined standard errors of 2^20 pseudo-random trajectories on the same 16 steps (the Euler bias stays in
    both); (c) the standard error at most half that of a GENERATE solve of the same budget 16·2^14 (the numpy restatement
    gave the ratio the golden file records)"""
    prob, steps = problem(True), 16
    qmc = hh.solve(prob, hh.QuasiMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(),
                                            hh.SobolConfig(sc.CONV_N_HESTON, steps=steps, randomizations=sc.CONV_R, seed=sc.CONV_SEED)))
    big = pseudo_random(prob, 2 ** 20, steps)
    same = pseudo_random(prob, sc.CONV_R * sc.CONV_N_HESTON, steps)
    print(f"\nHeston 16 steps: RQMC {qmc.price:.6f} ± {qmc.std_error:.2e}; 2^20 pseudo-random {big.price:.6f} ± {big.std_error:.2e}; "
          f"equal budget ± {same.std_error:.2e}: ratio {qmc.std_error / same.std_error:.3f}")
    assert abs(qmc.price - big.price) <= 4.0 * math.hypot(qmc.std_error, big.std_error)
    assert qmc.std_error <= 0.5 * same.std_error


def test_bridge_beats_incremental_on_64_steps(hhlib):
    prob, se = problem(True), {}
    for name, construction in (("bridge", hh.BrownianBridge()), ("incremental", hh.Incremental())):
        cfg = hh.SobolConfig(sc.CONV_N_HESTON, steps=64, randomizations=sc.CONV_R, seed=sc.CONV_SEED, construction=construction)
        se[name] = hh.solve(prob, hh.QuasiMonteCarlo(hh.HestonDynamics(), hh.EulerMaruyama(), cfg)).std_error
    print(f"\nHeston 64 steps: standard errors {se}")
    assert se["bridge"] < se["incremental"]


def test_forward_ad_and_finite_difference_deltas_agree(hhlib):
    """Lognormal Euler, 8 steps, N = 2^12, R = 8.  The discounted call payoff of a path is piecewise linear in S0 (the
    scheme's log spot is log S0 plus what does not depend on it), so a central difference has no truncation error on a
    path that does not cross the strike inside the bump: with the bump 1e-7 the band is ±1e-5 wide around K, which holds
    0.01 of the 32768 paths in expectation, and what remains is rounding, 1e-16·price/(2·bump·S0) ≈ 1e-10 — against the
    bar rel = 1e-6 tests/test_host_api.py holds a central difference to."""
    prob = problem(False)
    method = hh.QuasiMonteCarlo(hh.LognormalDynamics(), hh.EulerMaruyama(), hh.SobolConfig(2 ** 12, steps=8, randomizations=8, seed=sc.CONV_SEED))
    ad = hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.ForwardAD(), method).greek
    fd = hh.solve(hh.GreekProblem(prob, hh.SpotLens()), hh.FiniteDifference(1e-7), method).greek
    print(f"\ndelta: ForwardAD {ad:.10f}, FiniteDifference {fd:.10f}")
    assert 0.4 < ad < 0.8 and fd == pytest.approx(ad, rel=1e-6)


def test_exact_law_delta_converges_to_black_scholes(hhlib):
    """the delta of each randomisation by a central difference on its own points (the bumped solves share the seed); its
    mean within 4 standard errors, taken across the randomisations, of the closed form"""
    T, eps, S0 = hh.yearfrac(REF, EXP), 1e-4, sc.LOGNORMAL["S0"]
    _, delta = black_scholes(dict(sc.LOGNORMAL, T=T))
    method = hh.QuasiMonteCarlo(hh.LognormalDynamics(), hh.BlackScholesExact(),
                                hh.SobolConfig(sc.CONV_N_EXACT, randomizations=sc.CONV_R, seed=sc.CONV_SEED))
    up, dn = (hh.solve(problem(False, S0=S0 * (1 + s * eps)), method).estimates for s in (1, -1))
    per = (np.array(up) - np.array(dn)) / (2 * eps * S0)
    mean, se = sc.rqmc(per)
    print(f"\nexact-law delta {mean:.8f} ± {se:.2e}, Black–Scholes {delta:.8f}")
    fd = hh.solve(hh.GreekProblem(problem(False), hh.SpotLens()), hh.FiniteDifference(eps), method).greek
    assert fd == pytest.approx(mean, rel=1e-10)  # the FiniteDifference route is these plain solves
    assert se > 0.0 and abs(mean - delta) <= 4.0 * se


# ---- (f) the C-ABI's errors ----------------------------------------------------------------------------------------------------

def test_abi_errors_leave_the_context_usable(hhlib):
    ctx, lib, h = hhlib, hhlib.lib, hhlib.handle
    n, steps = 300, 4
    good = dev_fill(ctx, HES, -0.7, 1.0, steps, n, 0, sc.BRIDGE)
    dev = _ffi.DeviceBuffer(ctx, 8 * lib.hh_replay_elems(n, steps, HES))
    fill_args = dict(dyn=HES, rho=-0.7, T=1.0, steps=steps, n=n, off=0, seed=1, r=0, sh=1, con=sc.BRIDGE, dst=dev.ptr)
    pts_args = dict(dims=4, n=n, off=0, seed=1, r=0, sh=0, dst=dev.ptr)
    fill = lambda **kw: lib.hh_sobol_fill(h, *{**fill_args, **kw}.values())  # noqa: E731
    pts = lambda **kw: lib.hh_sobol_points(h, *{**pts_args, **kw}.values())  # noqa: E731
    cases = [
        ("fill.dst_null", lambda: fill(dst=None), INV), ("fill.rho", lambda: fill(rho=1.5), INV),
        ("fill.rho_nan", lambda: fill(rho=float("nan")), INV), ("fill.T", lambda: fill(T=0.0), INV),
        ("fill.steps0", lambda: fill(steps=0), INV), ("fill.n0", lambda: fill(n=0), INV),
        ("fill.past_2_32", lambda: fill(off=2 ** 32 - n + 1), INV), ("fill.offset", lambda: fill(off=2 ** 40), INV),
        ("fill.construction", lambda: fill(con=2), INV), ("fill.construction_neg", lambda: fill(con=-1), INV),
        ("fill.dims_heston", lambda: fill(steps=2049), UNS), ("fill.dims_lognormal", lambda: fill(dyn=GBM, steps=4097), UNS),
        ("points.dst_null", lambda: pts(dst=None), INV), ("points.dims0", lambda: pts(dims=0), INV),
        ("points.n0", lambda: pts(n=0), INV), ("points.past_2_32", lambda: pts(off=2 ** 32 - n + 1), INV),
        ("points.dims", lambda: pts(dims=4097), UNS),
    ]
    for name, call, want in cases:
        assert call() == want, name
        assert b"hh_sobol" in lib.hh_last_error(h), name
        np.testing.assert_array_equal(dev_fill(ctx, HES, -0.7, 1.0, steps, n, 0, sc.BRIDGE).view(np.uint64), good.view(np.uint64),
                                      err_msg=name)
    assert fill(off=2 ** 32 - n) == 0 and pts(off=2 ** 32 - n) == 0  # the last points there are
    ctx.synchronize()
    dev.free()
    assert lib.hh_sobol_fill(None, HES, -0.7, 1.0, steps, n, 0, 1, 0, 1, sc.BRIDGE, None) == INV
    v = (C.c_uint32 * 32)()
    assert lib.hh_sobol_directions(sc.MAX_DIMS, v) == INV and lib.hh_sobol_directions(0, None) == INV
