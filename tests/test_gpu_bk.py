"""Broadie–Kaya kernel (BASELINE config 4) against the numpy/scipy oracle on identical draws, and
against the Fourier price at full size.

Per-path parity is stated where it is DEFINED.  The inversion stops on |F(x) - u| <= 1e-4
(sample_from_cf.jl:110) and the series on |ϕ(hj)|/j < π·tol/2 (:88): a rounding-level difference in a
CF value can flip such a test and move that sample by up to ~atol/pdf.  Kernel and oracle therefore
both report, per trajectory, WHAT the search did (hh_bk_decisions: secant evaluations, finishing
branch, bisection iterations, series length).  Every trajectory whose decision word AND series length
agree must agree in value to the regime's conditioning bound (MATCHED_RTOL) — no allowance; the
trajectories where a decision flipped are counted, bounded in number and in size, separately."""
import ctypes as C
import math

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from oracle import analytic, bk_oracle
from tests import oracle_ffi as o

pytestmark = pytest.mark.gpu

PARAMS = {
    # benchmark problem H252 (test/agreement/montecarlo_heston.jl:13-22 parameters, T = 1)
    "h252": dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0,
                 strike=100.0, cp=1.0),
    # what montecarlo_heston.jl:161-170 actually runs: σ < 0, d ≈ 0.13, ν ≈ -0.93
    "q2": dict(S0=100.0, V0=1.5, kappa=0.04, theta=0.3, sigma=-0.6, rho=0.04, r=0.05, T=364 / 365,
               strike=100.0, cp=1.0),
    # the intended order of the same test
    "intended": dict(S0=100.0, V0=0.04, kappa=1.5, theta=0.04, sigma=0.3, rho=-0.6, r=0.05,
                     T=364 / 365, strike=100.0, cp=1.0),
    # low vol-of-vol: d = 32, ν = 15 (ratio recurrence), put
    "large_nu": dict(S0=100.0, V0=0.05, kappa=2.0, theta=0.04, sigma=0.1, rho=-0.3, r=0.02, T=0.5,
                     strike=105.0, cp=-1.0),
    # d = 128, ν = 63: arguments |z| ~ 50 between the series' plain range and the Hankel range of the
    # order — the ascending series where its terms do not cancel, else base order + ratio recurrence
    "nu_63": dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.05, rho=-0.3, r=0.02, T=1.0,
                  strike=100.0, cp=1.0),
    # ν = 15 at a monthly step: |z| ~ 200, beyond the order's Hankel threshold ν²/6 + 13
    "large_nu_short_T": dict(S0=100.0, V0=0.05, kappa=2.0, theta=0.04, sigma=0.1, rho=-0.3, r=0.02,
                             T=1.0 / 12.0, strike=100.0, cp=1.0),
    # integer Bessel orders: d = 4 (ν = 1, one ratio step on top of I_0) and d = 2 (ν = 0)
    "nu_one": dict(S0=100.0, V0=0.06, kappa=1.0, theta=0.09, sigma=0.3, rho=-0.4, r=0.02, T=1.5,
                   strike=95.0, cp=1.0),
    "nu_zero": dict(S0=100.0, V0=0.03, kappa=1.0, theta=0.045, sigma=0.3, rho=0.3, r=0.0, T=0.75,
                    strike=100.0, cp=-1.0),
    # short maturity: large Bessel arguments (Hankel branch), d < 1 with a large Poisson mean
    "short_T": dict(S0=100.0, V0=0.09, kappa=1.0, theta=0.02, sigma=0.5, rho=-0.5, r=0.01, T=0.02,
                    strike=100.0, cp=1.0),
}


def gpu_bk(ctx, prm, n, seed, offset=0):
    m = o.make_model(**prm)
    c = o.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, seeds=[seed], path_offset=offset)
    res = _ffi.hh_result()
    term = np.zeros(n)
    ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(m), C.byref(c), C.byref(res),
                                  term.ctypes.data))
    return res, term, m.discount


def gpu_decisions(ctx, n):
    dec, ln = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    ctx.check(ctx.lib.hh_bk_decisions(ctx.handle, n, dec.ctypes.data, ln.ctypes.data))
    return dec, ln


# Bound on a trajectory whose decision sequence matches the oracle's, by regime.  The reference takes
# the variance of ∫V from a second central difference of the CF with h = 1e-2 (sample_from_cf.jl:50-61):
# (ϕ₊ − 2ϕ₀ + ϕ₋) ≈ −(var+mean²)·1e-4 is formed from numbers of size 1, so fp64 rounding of ϕ (1e-16)
# reappears as a relative perturbation 1e-16 / ((var+mean²)·1e-4) of the moments, hence of the Fourier
# grid step, of every series term and of the sample.  With mean ≈ 0.02 (large_nu, short_T) that is
# ~1e-9..1e-7 whatever the implementation; it is what separates two correct fp64 implementations.
# Measured (tests/bk_parity_report.py, profiles/r03_c_bk_parity_report.txt; 2 x 600 trajectories per regime):
# h252 / q2 / intended / nu_one / nu_zero: every trajectory matched, worst 5.3e-9; large_nu: all matched,
# 6.1e-7; nu_63: 1 of 600 flipped, matched 4.6e-6; the two short-maturity regimes: 20-23 % flipped (their
# series are ~60 terms long and |ϕ|/j crosses the tolerance slowly: the LENGTH flips), matched 4.6e-5 / 6.7e-6,
# flipped 1.6e-4 at worst.  The bars below are those figures x 5.
MATCHED_RTOL = {"h252": 3e-8, "q2": 3e-8, "intended": 3e-8, "large_nu": 3e-6, "short_T": 4e-5,
                "nu_one": 3e-8, "nu_zero": 3e-8, "nu_63": 3e-5, "large_nu_short_T": 3e-4}
FLIPPED_RTOL = 1e-3   # a flipped stopping test moves the sample by ~atol/pdf at most
FLIPPED_SHARE = {"short_T": 0.35, "large_nu_short_T": 0.35}  # elsewhere: at most max(2, 1 %) trajectories


def assert_per_path_parity(name, term, ref, dec, ln, rtol=None):
    rel = np.abs(term - ref["terminal"]) / ref["terminal"]
    same = (dec == ref["decisions"]) & (ln == ref["series_len"])
    n = len(term)
    rtol = MATCHED_RTOL[name] if rtol is None else rtol
    assert np.all(np.isfinite(term))
    worst = np.max(rel[same]) if same.any() else 0.0
    assert worst <= rtol, (name, "matched trajectories", worst, int(np.argmax(np.where(same, rel, 0))))
    flipped = ~same
    assert flipped.sum() <= max(2, FLIPPED_SHARE.get(name, 0.01) * n), (name, int(flipped.sum()), n)
    if flipped.any():
        assert np.max(rel[flipped]) <= FLIPPED_RTOL, (name, "flipped trajectories", np.max(rel[flipped]))
    return int(flipped.sum()), worst


@pytest.mark.parametrize("name", list(PARAMS))
def test_bk_matches_oracle_per_path(hhlib, name):
    prm = PARAMS[name]
    n = 600
    res, term, D = gpu_bk(hhlib, prm, n, seed=2024, offset=5)
    dec, ln = gpu_decisions(hhlib, n)
    ref = bk_oracle.mc_solve(**prm, discount=D, n_paths=n, seed0=2024, path_offset=5)
    n_flipped, _ = assert_per_path_parity(name, term, ref, dec, ln)
    assert res.price == pytest.approx(ref["price"], rel=1e-4)
    st = ref["stats"]
    # the counters are sums of the decision words: they can differ by the flipped trajectories only
    assert abs(int(res.bk_newton_fail) - st["newton_fail"]) <= n_flipped
    assert abs(int(res.bk_maxguess_fallback) - st["maxguess"]) <= n_flipped
    assert int(res.bk_newton_fail) == int(np.sum((dec >> 8) & 3 != 0))
    if n_flipped == 0:
        assert res.bk_cf_terms == ref["cf_terms"]
    else:
        assert res.bk_cf_terms == pytest.approx(ref["cf_terms"], rel=0.05)


def test_bk_table_upload_survives_a_regrown_scratch(oracle):
    """the Bessel tables live inside the Broadie–Kaya scratch and are skipped when their key
    (address, order) is unchanged — a scratch that regrows at the SAME address (a larger term cache, same
    trajectory count) must not keep the key.  Fresh context: 32 terms, then 256, then 32 again."""
    ctx = _ffi.Context(0)
    prm = PARAMS["large_nu"]
    n = 400
    ref = bk_oracle.mc_solve(**prm, discount=o.make_model(**prm).discount, n_paths=n, seed0=77)
    try:
        for cache in (32, 256, 1024, 32):
            ctx.set_option(_ffi.HH_OPT_BK_TERM_CACHE, cache)
            _, term, _ = gpu_bk(ctx, prm, n, seed=77)
            dec, ln = gpu_decisions(ctx, n)
            assert_per_path_parity("large_nu", term, ref, dec, ln)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["h252", "q2", "large_nu"])
@pytest.mark.parametrize("on_device", [0, 1])
def test_bk_replay_of_the_callers_draws(hhlib, name, on_device):
    """HH_NOISE_REPLAY for Broadie–Kaya: the three draws per trajectory (V_T, u, Z — the reference's
    own, once julia/parity_replay.jl has exported them) come from the caller; here from scipy's
    noncentral chi-squared sampler, i.e. from no code of this repository.  Everything downstream
    (moments, CDF series, inverse_cdf, log S_T) against the oracle on the same draws."""
    import scipy.stats as st
    import torch
    prm = PARAMS[name]
    n = 500
    rng = np.random.default_rng(7)
    k, th, sg, T, V0 = prm["kappa"], prm["theta"], prm["sigma"], prm["T"], prm["V0"]
    em1 = -math.expm1(-k * T)
    d, lam = 4 * k * th / sg**2, 4 * k * math.exp(-k * T) * V0 / (sg**2 * em1)
    VT = sg**2 * em1 / (4 * k) * st.ncx2.rvs(d, lam, size=n, random_state=rng)  # heston.jl:128-131
    draws = np.ascontiguousarray(np.stack([VT, rng.uniform(size=n), rng.standard_normal(n)]))
    m = o.make_model(**prm)
    c = o.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, noise_mode=_ffi.HH_NOISE_REPLAY,
                      replay=draws.ravel())
    dev = None
    if on_device:
        dev = torch.from_numpy(draws.ravel().copy()).to("cuda:0")
        c.replay, c.replay_on_device = dev.data_ptr(), 1
    res = _ffi.hh_result()
    term = np.zeros(n)
    hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(res),
                                      term.ctypes.data))
    ref = bk_oracle.mc_solve(**prm, discount=m.discount, n_paths=n, seed0=0, replay=draws)
    assert_per_path_parity(name, term, ref, *gpu_decisions(hhlib, n))
    assert res.price == pytest.approx(ref["price"], rel=1e-4)
    # a buffer shorter than 3·n_paths is refused on the host, not read out of bounds on the device
    c2 = o.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, noise_mode=_ffi.HH_NOISE_REPLAY,
                       replay=draws.ravel()[:2 * n])
    assert hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c2), C.byref(res), None) == _ffi.HH_ERR_INVALID
    del dev


@pytest.mark.parametrize("n_a,n_b", [(300, 700), (16384, 256), (393216, 256)])
def test_bk_sharding_is_invisible(hhlib, n_a, n_b):
    """An ensemble in one solve and in two, bit for bit: the samples, and — read back after each solve for that
    solve's own trajectory count — the decision words and series lengths, which lie behind the term cache in the
    scratch buffer.  The cache has one column per lane of max(64, min(tiles, 1536)) workgroup slots: 64 tiles | 1
    tile and 1536 tiles | 1 tile are the smallest ensembles on both sides of the two branches of that rule."""
    prm = PARAMS["h252"]
    full = gpu_bk(hhlib, prm, n_a + n_b, 11)[1]
    dec, ln = gpu_decisions(hhlib, n_a + n_b)
    a = gpu_bk(hhlib, prm, n_a, 11)[1]
    dec_a, ln_a = gpu_decisions(hhlib, n_a)
    b = gpu_bk(hhlib, prm, n_b, 11, offset=n_a)[1]
    dec_b, ln_b = gpu_decisions(hhlib, n_b)
    np.testing.assert_array_equal(full, np.concatenate([a, b]))
    np.testing.assert_array_equal(dec, np.concatenate([dec_a, dec_b]))
    np.testing.assert_array_equal(ln, np.concatenate([ln_a, ln_b]))
    assert ln.min() >= 1  # a CDF series has its first term at least: the words were read where the chain wrote them


@pytest.mark.parametrize("name,cm_bound", [("h252", 400.0), ("q2", 32.0), ("intended", 200.0)])
def test_bk_full_size_vs_carr_madan(hhlib, name, cm_bound):
    """BASELINE config 4: 10^6 exact samples; the reference's own bar is rtol 2e-2 against
    CarrMadan (montecarlo_heston.jl:205,252) — here 4 standard errors."""
    prm = PARAMS[name]
    n = 1_000_000 if name == "h252" else 200_000
    res, term, D = gpu_bk(hhlib, prm, n, seed=99)
    cm = analytic.carr_madan_heston(prm["S0"], prm["strike"], prm["r"], prm["V0"], prm["kappa"],
                                    prm["theta"], prm["sigma"], prm["rho"], prm["T"],
                                    bound=cm_bound)
    assert res.price == pytest.approx(cm, rel=2e-2)
    assert abs(res.price - cm) < 4 * res.std_error + 2e-3 * cm
    # martingale: E[S_T] = S0 e^{rT}
    se_S = term.std() / math.sqrt(n)
    assert abs(term.mean() - prm["S0"] * math.exp(prm["r"] * prm["T"])) < 4 * se_S + 1e-3 * prm["S0"]
    assert res.n_paths_done == n and res.bk_maxguess_fallback < 0.01 * n


@pytest.mark.parametrize("term_cache", [32, 64, 256])
def test_bk_long_series_beyond_the_term_cache(hhlib, term_cache):
    """cf_tol = 1e-6 makes the CDF series 27-38 terms long.  With 32 cached Re ϕ_j per column
    (HH_OPT_BK_TERM_CACHE) most of them are beyond the cache: those trajectories run whole in the fall-back
    kernel, the tail recomputed from the stored unwrapped angle; with 64 or the default 256 they fit and are
    inverted on the cached terms.  Either way the oracle must be reproduced, which re-evaluates every term in
    every CDF call as the reference does."""
    prm = PARAMS["h252"]
    n = 300
    m = o.make_model(**prm)
    c = o.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, seeds=[31337])
    c.bk_cf_tol, c.bk_atol, c.bk_newton_maxiter = 1e-6, 1e-6, 20
    res = _ffi.hh_result()
    term = np.zeros(n)
    hhlib.set_option(_ffi.HH_OPT_BK_TERM_CACHE, term_cache)
    try:
        hhlib.check(hhlib.lib.hh_mc_solve(hhlib.handle, C.byref(m), C.byref(c), C.byref(res),
                                          term.ctypes.data))
    finally:
        hhlib.set_option(_ffi.HH_OPT_BK_TERM_CACHE, 256)
    with pytest.raises(_ffi.HedgehogMCError):
        hhlib.set_option(_ffi.HH_OPT_BK_TERM_CACHE, 4)
    ref = bk_oracle.mc_solve(**prm, discount=m.discount, n_paths=n, seed0=31337, cf_tol=1e-6,
                             atol=1e-6, maxiter_newton=20)
    assert res.bk_cf_terms / n > 100
    dec, ln = gpu_decisions(hhlib, n)
    # a series longer than the cache runs whole in the fall-back kernel — exactly those trajectories
    np.testing.assert_array_equal((dec >> 31).astype(bool), ln > term_cache, err_msg=str((dec[:8], ln[:8])))
    assert ((dec >> 31) != 0).any() == (term_cache < ln.max()) and ln.max() > 32
    assert_per_path_parity("h252", term, ref, dec & 0x7fffffff, ln, rtol=1e-8)
    assert res.bk_cf_terms == pytest.approx(ref["cf_terms"], rel=0.02)
    assert res.price == pytest.approx(ref["price"], rel=1e-5)


@pytest.mark.parametrize("name", ["h252", "q2", "intended"])
def test_bk_whole_trajectory_kernel_against_the_cached_chain(name):
    """With the smallest term cache (8) every series outgrows it, so EVERY trajectory runs whole in
    bk_fallback_kernel — a state machine around one CDF call site: secant, then the max_guess / bisection
    ladder — while the default cache sends the same trajectories through bk_cf_kernel's secant on cached
    terms and bk_ladder_kernel.  Two codings of inverse_cdf (sample_from_cf.jl:105-135) on the same draws:
    the same decisions (evaluations, finishing branch, bisection iterations), the same counters, and samples
    that differ only by where the series terms were rounded."""
    prm = PARAMS[name]
    n = 20_000  # ~2 % of H252's secants fail: some hundred ladders, bisections and max_guess exits
    ctx = _ffi.Context(0)
    try:
        out = {}
        for cache in (256, 8):
            ctx.set_option(_ffi.HH_OPT_BK_TERM_CACHE, cache)
            res, term, _ = gpu_bk(ctx, prm, n, seed=4242)
            dec, ln = gpu_decisions(ctx, n)
            out[cache] = (res, term, dec, ln)
    finally:
        ctx.close()
    (r1, t1, d1, l1), (r2, t2, d2, l2) = out[256], out[8]
    assert (d1 >> 31).sum() == 0 and ((d2 >> 31) == (l2 > 8)).all() and (l2 > 8).mean() > 0.99
    np.testing.assert_array_equal(l1, l2)
    same = (d1 & 0x7fffffff) == (d2 & 0x7fffffff)
    assert same.mean() > 0.999, (~same).sum()  # a stopping test within rounding of its threshold may flip
    np.testing.assert_allclose(t2[same], t1[same], rtol=1e-9)
    n_flip = int((~same).sum())
    for f in ("bk_newton_fail", "bk_bisect_fallback", "bk_maxguess_fallback"):
        assert abs(int(getattr(r1, f)) - int(getattr(r2, f))) <= n_flip, f
    assert r1.bk_newton_fail > 0 and r1.bk_bisect_fallback > 0
    assert r2.price == pytest.approx(r1.price, rel=1e-9 if n_flip == 0 else 1e-5)


def _bk_random_settings():
    from hypothesis import HealthCheck, settings
    # no shrinking phase: a failing example would re-run the (slow, pure-Python) oracle hundreds of times
    from hypothesis import Phase
    import os
    return settings(max_examples=int(os.environ.get("HH_BK_RANDOM_EXAMPLES", "40")), deadline=None, derandomize=True, database=None,
                    phases=[Phase.explicit, Phase.generate],
                    suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow,
                                           HealthCheck.filter_too_much])


try:
    from hypothesis import assume, given
    from hypothesis import strategies as st
except ImportError:  # pragma: no cover
    given = None

if given is not None:
    @_bk_random_settings()
    @given(kappa=st.floats(0.3, 4.0), theta=st.floats(0.01, 0.2), sigma=st.floats(0.05, 1.0),
           rho=st.sampled_from([-0.9, -0.5, 0.0, 0.4]), V0=st.floats(0.005, 0.3), T=st.floats(0.05, 3.0),
           cp=st.sampled_from([1.0, -1.0]), seed=st.integers(1, 2**31))
    def test_bk_random_models(hhlib, kappa, theta, sigma, rho, V0, T, cp, seed):
        """Random Heston parameters (Bessel orders ν = 2κθ/σ² − 1 from −0.98 to ~100, Bessel arguments
        from 0.1 to several hundred: every branch of hh_bessel.h's dispatch in situ) against the
        scipy / AMOS oracle on the same draws.  Per-path bars as in the fixed regimes above, at their
        loose end: the median sample within 1e-5, 95 % within 1e-3 (the moment differences and the
        |F(x) − u| <= 1e-4 stopping rule amplify rounding, see MATCHED_RTOL), the price within the mean
        sample difference (the payoff is 1-Lipschitz).

        Domain: where the REFERENCE works.  heston.jl:207 takes log(besseli(ν, ν_γ)) of the unscaled
        function, which overflows beyond |Re ν_γ| ≈ 709 (NaN samples); and the variance of ∫V comes
        from a second difference of ϕ with h = 1e-2 (sample_from_cf.jl:50-61) whose rounding is
        amplified by 1e-12 / (var + mean²) — with mean ∫V ≈ V0·T below ~2e-3 the reference's own
        moments are noise.  Such parameter sets are skipped; so are orders in the hundreds, where
        besseli underflows and the reference never leaves its series loop (OutsideReferenceRange): the
        kernels still return finite samples there (they carry log I_ν), which is all that can be
        asked."""
        em1 = -math.expm1(-kappa * T)
        nu_k = 4 * kappa * math.exp(-0.5 * kappa * T) / (sigma**2 * em1) * math.sqrt(V0 * 3 * max(V0, theta))
        assume(nu_k < 400.0 and min(V0, theta) * T > 2e-3)
        prm = dict(S0=100.0, V0=V0, kappa=kappa, theta=theta, sigma=sigma, rho=rho, r=0.02, T=T,
                   strike=100.0, cp=cp)
        n = 120
        res, term, D = gpu_bk(hhlib, prm, n, seed=seed)
        try:
            ref = bk_oracle.mc_solve(**prm, discount=D, n_paths=n, seed0=seed)
        except bk_oracle.OutsideReferenceRange:
            # ν in the hundreds: I_ν(z) itself underflows, the reference's log(besseli(…)) is -Inf and its
            # series loop never ends (the oracle raises instead); the kernels carry log I_ν and go on
            assert np.all(np.isfinite(term)) and np.all(term > 0)
            return
        assert np.all(np.isfinite(term)) and np.all(term > 0)
        rel = np.abs(term - ref["terminal"]) / ref["terminal"]
        nu = 2 * kappa * theta / sigma**2 - 1
        assert np.median(rel) < 1e-5, (nu, np.median(rel), np.sort(rel)[-5:])  # 2e-6 at ν = -0.987, mean ∫V = 0.03
        assert np.mean(rel > 1e-3) <= 0.05, (nu, np.sort(rel)[-8:])
        # the payoff is 1-Lipschitz in S_T: the prices cannot differ by more than the mean sample difference
        assert abs(res.price - ref["price"]) <= D * np.mean(np.abs(term - ref["terminal"])) * (1 + 1e-9) + 1e-9


def test_bk_tail_kernel_beyond_its_first_turn_of_tiles():
    """More than 64 x 256 tiles (4.2·10^6 trajectories), a term cache that a share of the series outgrows: a tail
    workgroup then looks at its tiles in more than one turn of 256 (for_long_tiles), every tail workgroup has work, the
    reducers wait for all of them — and a second model that shares the chain (a bumped spot: bk_refinish_kernel) rebuilds
    those records in the same order.  Against the same ensemble with the default cache, where no series is too long:
    the same decisions and samples up to where the series terms were rounded; and the shared chain against each model's
    own solve, bit for bit."""
    prm = PARAMS["h252"]
    n = 256 * 16384 + 777
    ctx = _ffi.Context(0)
    try:
        m = o.make_model(**prm)
        c = o.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, seeds=[99])
        c.bk_cf_tol = 2e-5  # series of ~20-30 terms
        out = {}
        for cache in (256, 24):
            ctx.set_option(_ffi.HH_OPT_BK_TERM_CACHE, cache)
            res = _ffi.hh_result()
            term = np.zeros(n)
            ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(m), C.byref(c), C.byref(res), term.ctypes.data))
            dec, ln = gpu_decisions(ctx, n)
            out[cache] = (res, term, dec, ln)
        (r1, t1, d1, l1), (r2, t2, d2, l2) = out[256], out[24]
        long_ = (d2 >> 31).astype(bool)
        assert (d1 >> 31).sum() == 0 and (long_ == (l2 > 24)).all()
        assert 0.02 < long_.mean() < 0.98, long_.mean()  # some series fit, some do not: both kernels have work everywhere
        tiles_with_long = np.unique(np.nonzero(long_)[0] // 256)
        assert tiles_with_long.max() >= 64 * 256  # … beyond a tail workgroup's first turn
        np.testing.assert_array_equal(l1, l2)
        same = (d1 & 0x7fffffff) == (d2 & 0x7fffffff)
        assert same.mean() > 0.999
        np.testing.assert_allclose(t2[same], t1[same], rtol=1e-9)
        assert r2.price == pytest.approx(r1.price, rel=1e-6)
        # the shared chain with the small cache: records of the tail workgroups rebuilt by bk_refinish_kernel
        models = [m, o.make_model(**dict(prm, S0=prm["S0"] * 1.001))]
        res2 = (_ffi.hh_result * 2)()
        ctx.check(ctx.lib.hh_mc_solve_multi(ctx.handle, (_ffi.hh_model * 2)(*models), 2, C.byref(c), res2, None))
        for k in range(2):
            own = _ffi.hh_result()
            ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(models[k]), C.byref(c), C.byref(own), None))
            assert (res2[k].price, res2[k].sumsq_payoff, res2[k].bk_cf_terms) == (own.price, own.sumsq_payoff, own.bk_cf_terms)
        assert res2[0].price == r2.price
    finally:
        ctx.close()
