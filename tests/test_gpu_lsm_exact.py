"""The LSM induction (hh_lsm.hip) against exact sums and the high-precision fit of oracle/lsm_exact.py.

a. Sums through the phases (hh_lsm_shard_begin / _phase / _finish, one rank): the in-the-money count exactly,
   Σx, Σx², Σ z^k and Σ z^k y within γ_h Σ|term| of the exact sum of the same fp64 terms, h the depth of the
   summation tree (lsm_exact.tree_depth: Q − 1 + 6 + 7 + ceil(nch/256) − 1 + 6 + 3).  The state behind every
   Σ z^k y is known because the host forces the decisions: a row fed B = 0 fits cont = 0 and exercises every
   in-the-money trajectory; a row whose statistics are fed with n = 0 has no fit and exercises none.
b. One regression per row: the grid [S0, x_t, S_N] with step_discount = D^(N−t) runs exactly one regression
   (hh_lsm_solve_grid, n_steps = 2); its stopping times show every decision at x_t.  They must equal the exact
   decisions wherever |pay − cont*| > δ_i.
c. Hand-made rows through the same probe.
d. Matched chain: the host drives the whole induction through the phases with exact power sums and exact moment
   sums of its own high-precision state, so that no flipped decision cascades into later fits.  Every trajectory
   without a near-tie at any row must end with the host's stopping time and value.
"""
import ctypes as C
import math
import time
import zlib

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from oracle import lsm_exact as L
from tests import oracle_ffi as o

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
U = L.U


@pytest.fixture(scope="module")
def ctx():
    return _ffi.Context(0)


def gamma(h):
    return h * U / (1 - h * U)


def disc_table(D, n):
    return np.exp(math.log(D) * np.arange(n + 1, dtype=np.float64))


class Phases:
    """One rank of the sharded induction, the exchange vector in device memory."""

    def __init__(self, ctx, m, c, degree, D, steps):
        self.ctx, self.degree, self.steps = ctx, degree, steps
        self.x = torch.zeros(ctx.lib.hh_lsm_shard_xchg_elems(steps, degree), dtype=torch.float64, device="cuda")
        self.m, self.c = m, c
        torch.cuda.synchronize()
        ctx.check(ctx.lib.hh_lsm_shard_begin(ctx.handle, C.byref(m), C.byref(c), degree, D, self.x.data_ptr()))
        ctx.synchronize()
        self.stats = self._out((steps + 1) * 3).reshape(steps + 1, 3)

    def _out(self, n):
        return self.x[:n].cpu().numpy().copy()

    def _run(self, phase, t, vin, nout):
        self.x.zero_()
        self.x[:len(vin)] = torch.from_numpy(np.ascontiguousarray(vin, dtype=np.float64).ravel()).cuda()
        torch.cuda.synchronize()
        self.ctx.check(self.ctx.lib.hh_lsm_shard_phase(self.ctx.handle, phase, t, self.x.data_ptr(),
                                                       self.x.data_ptr()))
        self.ctx.synchronize()
        return self._out(nout) if nout else None

    def pow(self, stats):
        nv = 2 * self.degree + 1
        return self._run(_ffi.HH_LSM_PHASE_POW, 0, stats.ravel(), (self.steps + 1) * nv).reshape(self.steps + 1, nv)

    def init(self, P):
        return self._run(_ffi.HH_LSM_PHASE_INIT, 0, P.ravel(), self.degree + 1 if self.steps >= 2 else 0)

    def step(self, t, B):
        return self._run(_ffi.HH_LSM_PHASE_STEP, t, B, self.degree + 1 if t >= 2 else 0)

    def finish(self, ntot):
        acc = torch.zeros(_ffi.HH_ACC_LEN, dtype=torch.float64, device="cuda")
        tau, val = np.zeros(ntot, dtype=np.int32), np.zeros(ntot)
        grid = np.zeros((self.steps + 1, ntot))
        torch.cuda.synchronize()
        self.ctx.check(self.ctx.lib.hh_lsm_shard_finish(self.ctx.handle, acc.data_ptr(), tau.ctypes.data,
                                                        val.ctypes.data, grid.ctypes.data, None, None))
        res = _ffi.hh_lsm_result()
        acc_h = np.ascontiguousarray(acc.cpu().numpy())
        assert self.ctx.lib.hh_lsm_finalize(acc_h.ctypes.data, C.byref(res)) == 0
        return tau, val, grid, res


def gbm_problem(n, steps, anti, cp, K, seed, S0=100.0, r=0.05, sigma=0.25, T=0.75):
    seeds = np.random.default_rng(seed).integers(0, 2**63, n).astype(np.uint64)
    m = o.make_model(S0=S0, sigma=sigma, r=r, T=T, strike=K, cp=cp)
    c = o.make_config(0, 1, n, steps, antithetic=anti, seeds=seeds)
    return m, c, math.exp(-r * T / steps), seeds


def payoff(cp, x, K):
    m = cp * (x - K)
    return np.where(m > 0.0, m, 0.0)


# ---- a. sums through the phases -------------------------------------------------------------------------------

SIZES = [(1, 0, 3, -1.0, 5), (511, 0, 8, 1.0, 5), (1023, 0, 1, -1.0, 6), (1024, 1, 5, -1.0, 6),
         (1025, 0, 2, 1.0, 5), (2**18 - 1, 0, 7, -1.0, 3), (2**18, 1, 4, -1.0, 3), (2**18 + 1, 0, 6, 1.0, 3),
         (300_001, 0, 8, -1.0, 3), (300_000, 1, 3, 1.0, 4)]


@pytest.mark.parametrize("ntot,anti,degree,cp,steps", SIZES, ids=lambda v: str(v))
def test_sums_through_the_phases(ctx, ntot, anti, degree, cp, steps):
    n = ntot // 2 if anti else ntot
    K = 100.0 if cp < 0 else 98.0
    m, c, D, _ = gbm_problem(n, steps, anti, cp, K, seed=ntot + degree)
    ph = Phases(ctx, m, c, degree, D, steps)
    rng = np.random.default_rng(ntot)
    # rows with decisions forced: 'E' every in-the-money trajectory exercises (B = 0), 'N' none (n fed as 0)
    regime = {t: ("E" if rng.random() < 0.5 else "N") for t in range(1, steps)}
    stats_in = ph.stats.copy()
    for t, g in regime.items():
        if g == "N":
            stats_in[t, 0] = 0.0
    P = ph.pow(stats_in)
    outs = {steps - 1: ph.init(P)} if steps >= 2 else {}
    for t in range(steps - 1, 0, -1):
        B = np.zeros(degree + 1)
        o_ = ph.step(t, B)
        if t >= 2:
            outs[t - 1] = o_
    tau_d, val_d, grid, res = ph.finish(ntot)
    h, gam = L.tree_depth(ntot), gamma(L.tree_depth(ntot))
    bit_equal = []

    def check(got, terms, extra_ulps=None, what=""):
        for k in range(terms.shape[0]):
            want = L.exact_sum(terms[k])
            tol = (gam + (extra_ulps[k] if extra_ulps is not None else 0.0) * U) * float(np.sum(np.abs(terms[k])))
            assert abs(got[k] - want) <= tol, (what, k, float(got[k]), float(want), tol)
        bit_equal.append(np.array_equal(got, L.tree_sum(terms)))

    # statistics of every row: n exactly
    for row in range(steps + 1):
        x = grid[row]
        itm = cp * (x - K) > 0.0
        xm = np.where(itm, x, 0.0)
        assert ph.stats[row, 0] == itm.sum()
        check(ph.stats[row], np.stack([itm.astype(float), xm, xm * xm]), what=f"stats row {row}")
        mu, isd = L.rowstat(*stats_in[row])
        z = L.device_z(x, mu, isd)
        pw = np.where(itm, L.device_powers(z, 2 * degree), 0.0)
        assert P[row, 0] == itm.sum(), row
        check(P[row], pw, what=f"power sums row {row}")
    # the stopping state row by row, as the forced decisions leave it
    disc = disc_table(D, steps)
    tau = np.full(ntot, steps)
    val = payoff(cp, grid[steps], K)
    extra = np.arange(degree + 1) * 2 + 8.0   # y's discount factor (device exp) and the products that follow
    for t in range(steps - 1, 0, -1):
        if t == steps - 1 and steps >= 2:
            r = steps - 1
            mu, isd = L.rowstat(*stats_in[r])
            itm = cp * (grid[r] - K) > 0.0
            y = disc[tau - r] * val
            terms = np.where(itm, L.device_moment_terms(L.device_z(grid[r], mu, isd), y, degree), 0.0)
            check(outs[r], terms, extra, what=f"init moments row {r}")
        itm = cp * (grid[t] - K) > 0.0
        if regime[t] == "E":
            tau = np.where(itm, t, tau)
            val = np.where(itm, cp * (grid[t] - K), val)
        if t >= 2:
            r = t - 1
            mu, isd = L.rowstat(*stats_in[r])
            itm = cp * (grid[r] - K) > 0.0
            y = disc[tau - r] * val
            terms = np.where(itm, L.device_moment_terms(L.device_z(grid[r], mu, isd), y, degree), 0.0)
            check(outs[r], terms, extra, what=f"step {t}: moments row {r}")
    np.testing.assert_array_equal(tau_d, tau)
    np.testing.assert_array_equal(val_d, val)
    d = np.exp(math.log(D) * tau) * val
    mean = math.fsum(d) / ntot
    assert res.n_paths_total == ntot
    assert res.price == pytest.approx(mean, rel=1e-13, abs=1e-300)
    if ntot > 1:
        var = (math.fsum(d * d) - ntot * mean * mean) / (ntot - 1)
        assert res.std_error == pytest.approx(math.sqrt(max(var, 0.0) / ntot), rel=1e-13, abs=1e-300)
    print(f"\nntot={ntot}: depth {h}; sums equal to the tree restatement bit for bit: "
          f"{sum(bit_equal)} of {len(bit_equal)}")


# ---- b/c. one regression per row ----------------------------------------------------------------------------

def probe(ctx, S0, x, SN, K, cp, D, degree):
    """tau[i] == 1: the device exercised trajectory i at x (the middle row of [S0, x, S_N])."""
    ntot = len(x)
    g = np.ascontiguousarray(np.stack([np.full(ntot, S0), x, SN]))
    dev = torch.from_numpy(g).cuda()
    torch.cuda.synchronize()
    m = o.make_model(S0=S0, sigma=0.2, r=0.0, T=1.0, strike=K, cp=cp)
    tau, val = np.zeros(ntot, dtype=np.int32), np.zeros(ntot)
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve_grid(ctx.handle, C.byref(m), dev.data_ptr(), ntot, 2, degree, D,
                                        C.byref(res), tau.ctypes.data, val.ctypes.data))
    return tau


def probe_row(ctx, S0, x, SN, K, cp, D, degree):
    """(mismatches outside δ, decisions inside δ, in-the-money count, ambiguous row)"""
    tau = probe(ctx, S0, x, SN, K, cp, D, degree)
    itm = cp * (x - K) > 0.0
    assert np.all(tau[~itm] == 2)                     # out of the money (x == K included): never exercised
    xi = x[itm]
    d1 = math.exp(math.log(D))
    y = d1 * payoff(cp, SN[itm], K)
    fit = L.exact_row_fit(xi, y, degree, h=L.tree_depth(len(x)), e_y=5.0)
    ex, near = L.decisions(cp * (xi - K), fit)
    dev = tau[itm] == 1
    bad = int(np.sum((dev != ex) & ~near))
    return bad, int(near.sum()), int(itm.sum()), fit.ambiguous


def _grids(ctx):
    out = []
    # exact GBM (hh_lsm_solve's grid), antithetic
    n, N = 1500, 8
    m, c, D, _ = gbm_problem(n, N, 1, -1.0, 100.0, seed=5, sigma=0.35, T=1.0)
    g = np.zeros((N + 1, 2 * n))
    tau, val = np.zeros(2 * n, dtype=np.int32), np.zeros(2 * n)
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve(ctx.handle, C.byref(m), C.byref(c), 3, D, C.byref(res), tau.ctypes.data,
                                   val.ctypes.data, g.ctypes.data))
    out.append(("gbm", g, 100.0, -1.0, D))
    # deep out of the money: from 8 to ~100 in-the-money spots in one tail, where the pivots of the degree 6-8 fits
    # come closest to the drop rule
    n, N = 1000, 8
    m, c, D, _ = gbm_problem(n, N, 1, -1.0, 80.0, seed=13, sigma=0.25, T=0.5)
    g = np.zeros((N + 1, 2 * n))
    tau, val = np.zeros(2 * n, dtype=np.int32), np.zeros(2 * n)
    ctx.check(ctx.lib.hh_lsm_solve(ctx.handle, C.byref(m), C.byref(c), 3, D, C.byref(res), tau.ctypes.data,
                                   val.ctypes.data, g.ctypes.data))
    out.append(("gbm-deep", g, 80.0, -1.0, D))
    # Euler Heston, spot and log rows
    H = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03)
    for state, K in ((_ffi.HH_PATH_SPOT, 105.0), (_ffi.HH_PATH_LOG, 4.65)):
        n, N = 2000, 6
        mm = o.make_model(**H, T=0.75, strike=K, cp=-1.0)
        cc = o.make_config(_ffi.HH_HESTON, _ffi.HH_EULER_MARUYAMA, n, N, antithetic=0,
                           seeds=np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        g = np.full((N + 1, n), np.nan)
        r_ = _ffi.hh_result()
        ctx.check(ctx.lib.hh_euler_grid(ctx.handle, C.byref(mm), C.byref(cc), state, g.ctypes.data, None, 0,
                                        C.byref(r_)))
        out.append(("euler-log" if state == _ffi.HH_PATH_LOG else "euler-spot", g, K, -1.0,
                    math.exp(-0.03 * 0.75 / N)))
    # Broadie–Kaya
    n, N = 800, 4
    seeds = np.random.default_rng(9).integers(0, 2**63, n).astype(np.uint64)
    mm = o.make_model(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0,
                      strike=100.0, cp=-1.0)
    cc = o.make_config(_ffi.HH_HESTON, _ffi.HH_BROADIE_KAYA, n, N, seeds=seeds)
    g = np.zeros((N + 1, n))
    r_ = _ffi.hh_result()
    ctx.check(ctx.lib.hh_heston_exact_grid(ctx.handle, C.byref(mm), C.byref(cc), g.ctypes.data, None, 0,
                                           C.byref(r_)))
    out.append(("bk", g, 100.0, -1.0, math.exp(-0.03 / N)))
    return out


def test_one_regression_per_row(ctx):
    t0 = time.time()
    lines, total_near, total_itm = [], 0, 0
    for name, g, K, cp, Dstep in _grids(ctx):
        N = g.shape[0] - 1
        for t in range(1, N):
            for degree in range(1, 9):
                bad, near, nitm, amb = probe_row(ctx, g[0, 0], g[t], g[N], K, cp, Dstep ** (N - t), degree)
                assert bad == 0, (name, t, degree, bad)
                assert amb or near <= 0.01 * nitm + 2, (name, t, degree, near, nitm)
                total_near += near
                total_itm += nitm
                if near:
                    lines.append(f"{name} row {t} degree {degree}: {near} of {nitm} inside δ{' (ambiguous)' if amb else ''}")
    print("\n" + "\n".join(lines) + f"\nall rows: {total_near} of {total_itm} decisions inside δ "
          f"({time.time() - t0:.1f} s)")


HAND = []
for _deg in range(1, 9):
    HAND += [(f"itm-{k}", _deg) for k in range(0, _deg + 2)]
    HAND += [(f"distinct-{k}", _deg) for k in range(1, _deg + 2)]
    HAND += [("equal", _deg), ("spread-1e-9", _deg), ("at-strike", _deg), ("level-1e4", _deg)]


@pytest.mark.parametrize("kind,degree", HAND, ids=lambda v: str(v))
def test_hand_made_rows(ctx, kind, degree):
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{degree}".encode()))
    K, cp, D, n = 100.0, -1.0, 0.99, 1200
    x = K + rng.uniform(1.0, 30.0, n)                      # out of the money by default
    if kind.startswith("itm-"):
        k = int(kind[4:])
        x[:k] = K - rng.uniform(0.5, 20.0, k)
    elif kind.startswith("distinct-"):
        lv = K - 2.0 - 1.5 * np.arange(int(kind[9:]))
        x[:500] = lv[rng.integers(0, len(lv), 500)]
    elif kind == "equal":
        x[:500] = 93.0
    elif kind == "spread-1e-9":
        x[:500] = 90.0 * (1.0 + 1e-9 * rng.standard_normal(500))
    elif kind == "at-strike":
        x[:300] = K
        x[300:700] = K - rng.uniform(0.0, 15.0, 400)
    elif kind == "level-1e4":
        K = 1.0e4
        x = K * np.exp(0.15 * rng.standard_normal(n))
    SN = x * np.exp(0.1 * rng.standard_normal(n))
    bad, near, nitm, amb = probe_row(ctx, K, x, SN, K, cp, D, degree)
    assert bad == 0
    print(f"\n{kind} degree {degree}: {near} of {nitm} inside δ{' (ambiguous)' if amb else ''}")
    # a row is ambiguous when a column lies within its rounding margin of the drop threshold (fewer distinct
    # spots than coefficients, and the interpolating columns near the threshold): every decision counts as a tie
    if not amb:
        assert near <= 0.01 * nitm + 2


# ---- d. matched chain ----------------------------------------------------------------------------------------

def matched_chain(ctx, n, steps, anti, cp, K, degree, S0, r, sigma, T, seed):
    m, c, D, seeds = gbm_problem(n, steps, anti, cp, K, seed, S0=S0, r=r, sigma=sigma, T=T)
    ntot = n * (2 if anti else 1)
    grid = np.zeros((steps + 1, ntot))
    tau0, val0 = np.zeros(ntot, dtype=np.int32), np.zeros(ntot)
    res = _ffi.hh_lsm_result()
    ctx.check(ctx.lib.hh_lsm_solve(ctx.handle, C.byref(m), C.byref(c), degree, D, C.byref(res),
                                   tau0.ctypes.data, val0.ctypes.data, grid.ctypes.data))
    ph = Phases(ctx, m, c, degree, D, steps)
    stats, P, zs = np.zeros((steps + 1, 3)), np.zeros((steps + 1, 2 * degree + 1)), {}
    for row in range(steps + 1):
        itm = cp * (grid[row] - K) > 0.0
        x = grid[row][itm]
        stats[row] = [len(x), float(L.exact_sum(x)), float(L.exact_sum_sq(x))]
        z = L.device_z(x, *L.rowstat(*stats[row]))
        zs[row] = (itm, z)
        if len(x):
            with L.mpmath.workdps(L.DPS):
                P[row] = [float(v) for v in L.exact_power_sums(z, kmax=2 * degree)]
    ph.pow(stats)
    ph.init(P)
    disc = disc_table(D, steps)
    tau, val = np.full(ntot, steps), payoff(cp, grid[steps], K)
    tie = np.zeros(ntot, dtype=bool)
    for t in range(steps - 1, 0, -1):
        itm, z = zs[t]
        B = np.zeros(degree + 1)
        if itm.any():
            y = disc[tau[itm] - t] * val[itm]
            with L.mpmath.workdps(L.DPS):
                B[:] = [float(v) for v in L.exact_power_sums(z, y, kmax=degree)]
            fit = L.exact_row_fit(grid[t][itm], y, degree, h=1, e_y=0.0, z=z)
            pay = cp * (grid[t][itm] - K)
            ex, near = L.decisions(pay, fit)
            idx = np.nonzero(itm)[0]
            tie[idx[near]] = True
            tau[idx[ex]] = t
            val[idx[ex]] = pay[ex]
        ph.step(t, B)
    tau_d, val_d, _, _ = ph.finish(ntot)
    ok = ~tie
    bad = int(np.sum((tau_d != tau)[ok] | (val_d != val)[ok]))
    return bad, int(tie.sum()), ntot, int(np.sum(tau0 != tau))


CHAIN = [(3000, 30, 1, -1.0, 100.0, 5), (1025, 7, 0, -1.0, 110.0, 3), (3000, 30, 0, 1.0, 100.0, 4),
         (1025, 7, 1, -1.0, 40.0, 2), (700, 1, 0, -1.0, 100.0, 1), (1025, 7, 0, -1.0, 100.0, 6),
         (1025, 7, 1, -1.0, 110.0, 7), (3000, 12, 0, -1.0, 100.0, 8), (700, 9, 1, 1.0, 100.0, 8)]


@pytest.mark.parametrize("n,steps,anti,cp,K,degree", CHAIN, ids=lambda v: str(v))
def test_matched_chain(ctx, n, steps, anti, cp, K, degree):
    S0, r = (120.0 if cp > 0 else 100.0), (0.15 if cp > 0 else 0.05)
    bad, ties, ntot, vs_solve = matched_chain(ctx, n, steps, anti, cp, K, degree, S0, r, 0.25, 0.75,
                                              seed=n + steps)
    print(f"\n{ntot} trajectories, degree {degree}: {ties} with a near-tie; "
          f"{vs_solve} stopping times differ from hh_lsm_solve's own chain")
    assert bad == 0
    assert ties <= 0.002 * ntot + 2


try:
    from hypothesis import HealthCheck, Phase, given, settings
    from hypothesis import strategies as st
except ImportError:  # pragma: no cover
    given = None

if given is not None:
    @settings(max_examples=8, deadline=None, derandomize=True, database=None,
              phases=[Phase.explicit, Phase.generate],
              suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
    @given(n=st.sampled_from([64, 257, 1000, 1025, 3000]), steps=st.integers(1, 20),
           degree=st.integers(1, 8), anti=st.booleans(), cp=st.sampled_from([1.0, -1.0]),
           S0=st.floats(20.0, 200.0), moneyness=st.floats(0.6, 1.5), r=st.floats(0.0, 0.15),
           sigma=st.floats(0.05, 0.8), T=st.floats(0.05, 3.0), seed=st.integers(0, 2**31))
    def test_matched_chain_random_problems(ctx, n, steps, degree, anti, cp, S0, moneyness, r, sigma, T, seed):
        """The distribution of test_gpu_lsm.py::test_lsm_random_problems: zero unexplained mismatches."""
        bad, ties, ntot, _ = matched_chain(ctx, n, steps, int(anti), cp, S0 * moneyness, degree, S0, r, sigma,
                                           T, seed)
        assert bad == 0, (bad, ties, ntot)
