"""The argument errors of the C-ABI, pinned: every row is one bad call and the (status, hh_last_error) it must
report — the first problem of the call, in the order the entry point checks.  Covers NULL arguments, out-of-range
degree / n_steps / n_payoffs / path_state, unsupported dynamics/strategy pairs, a short seeds_len, a per-payoff
Carr–Madan error (which names the payoff), the shard calls without hh_lsm_shard_begin, and the hh_mgpu_* argument
errors (hh_mgpu_last_error)."""
import ctypes as C

import numpy as np
import pytest

from hedgehog_jl_amd import _ffi

pytestmark = pytest.mark.gpu

INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
LOGN, HEST = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON
EULER, EXACT, BK = _ffi.HH_EULER_MARUYAMA, _ffi.HH_EXACT_LAW, _ffi.HH_BROADIE_KAYA
SEEDS = np.arange(1, 11, dtype=np.uint64)
LSM_RANGE = "LSM: n_paths, n_steps >= 1, 1 <= degree <= 8"
LSM_PAIR = "LSM needs LognormalDynamics + BlackScholesExact or HestonDynamics + HestonBroadieKaya paths"
CM_BOUND = "%s: bound/alpha must be <= 196608 (1024 sub-panels of half-width 0.75 alpha per lane)"
NULL = None


def cfg(dyn=HEST, strat=EULER, n=10, steps=4, seeds=SEEDS, **kw):
    return _ffi.make_config(dyn, strat, n, steps, seeds=seeds, **kw)


def ref(x):
    return NULL if x is None else C.byref(x)


class Env:
    """What the rows call with: a context of their own, host-sum multi-GPU contexts of one and of two shards (both on
    device 0), and real device buffers (nothing is read from them: every row fails before a launch)."""

    def __init__(self):
        self.ctx = _ffi.Context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.mg1 = _ffi.MultiGpu([0], _ffi.HH_MGPU_HOST_SUM)
        self.mg2 = _ffi.MultiGpu([0, 0], _ffi.HH_MGPU_HOST_SUM)
        self.dev = _ffi.DeviceBuffer(self.ctx, 1 << 16)
        self.host = np.zeros(1 << 13)
        self.res = (_ffi.hh_result * 4)()
        self.lres = _ffi.hh_lsm_result()

    def close(self):
        self.dev.free()
        self.mg1.close()
        self.mg2.close()
        self.ctx.close()


def arr(*v):
    return np.array(v, dtype=np.float64)


def cm_args(e, strikes=(90.0, 100.0, 110.0), cps=(1.0, -1.0, 1.0), n=3):
    k = [arr(*strikes), arr(*cps), arr(1.0, 1.0, 1.0), arr(0.03, 0.03, 0.03), arr(0.97, 0.97, 0.97)]
    e._keep = k
    return [x.ctypes.data for x in k] + [n]


def m_():
    return _ffi.make_model()


# (id, call(env) -> status, expected status, expected text, which context reports it: "ctx" or "mg1" / "mg2")
def rows():
    r = []

    def add(i, fn, code, text, who="ctx"):
        r.append((i, fn, code, text, who))

    # hh_mc_solve / hh_mc_accumulate
    add("mc_solve.out_null", lambda e: e.lib.hh_mc_solve(e.h, ref(m_()), ref(cfg()), NULL, NULL), INV, "result is NULL")
    add("mc_solve.model_null", lambda e: e.lib.hh_mc_solve(e.h, NULL, ref(cfg()), e.res, NULL), INV,
        "model/config is NULL")
    add("mc_solve.n_steps", lambda e: e.lib.hh_mc_solve(e.h, ref(m_()), ref(cfg(steps=4 * 65535 + 1)), e.res, NULL),
        INV, "n_steps too large (max 262140)")
    add("mc_solve.pair", lambda e: e.lib.hh_mc_solve(e.h, ref(m_()), ref(cfg(LOGN, BK, steps=1)), e.res, NULL), UNS,
        "no simulation method for dynamics 0 with strategy 2")
    add("mc_solve.seeds_len", lambda e: e.lib.hh_mc_solve(e.h, ref(m_()), ref(cfg(seeds=SEEDS[:5])), e.res, NULL), INV,
        "Number of seeds (5) must be >= number of trajectories (10)")
    add("mc_accumulate.accum_null", lambda e: e.lib.hh_mc_accumulate(e.h, ref(m_()), ref(cfg()), NULL, NULL), INV,
        "accum_dev is NULL")
    # hh_mc_solve_multi
    two = lambda: (_ffi.hh_model * 2)(m_(), _ffi.make_model(S0=101.0))  # noqa: E731
    add("mc_solve_multi.out_null", lambda e: e.lib.hh_mc_solve_multi(e.h, two(), 2, ref(cfg()), NULL, NULL), INV,
        "hh_mc_solve_multi: 1 .. 16 models and their results")
    add("mc_solve_multi.n_models", lambda e: e.lib.hh_mc_solve_multi(e.h, two(), 17, ref(cfg()), e.res, NULL), INV,
        "hh_mc_solve_multi: 1 .. 16 models and their results")
    add("mc_solve_multi.partials", lambda e: e.lib.hh_mc_solve_multi(e.h, two(), 2, ref(cfg(n_partials=1)), e.res,
                                                                     NULL),
        UNS, "several models in one pass carry no dual partials (n_partials must be 0)")
    # hh_mc_solve_basket
    k, s = arr(90.0, 110.0), arr(1.0, -1.0)
    add("mc_solve_basket.out_null", lambda e: e.lib.hh_mc_solve_basket(e.h, ref(m_()), ref(cfg()), k.ctypes.data,
                                                                       s.ctypes.data, 2, NULL, NULL),
        INV, "result is NULL")
    add("mc_solve_basket.n_payoffs", lambda e: e.lib.hh_mc_solve_basket(e.h, ref(m_()), ref(cfg()), k.ctypes.data,
                                                                        s.ctypes.data, 0, e.res, NULL),
        INV, "hh_mc_accumulate_basket: bad arguments")
    add("mc_solve_basket.n_payoffs_max", lambda e: e.lib.hh_mc_solve_basket(e.h, ref(m_()), ref(cfg()), k.ctypes.data,
                                                                            s.ctypes.data, 65536, e.res, NULL),
        INV, "hh_mc_accumulate_basket: bad arguments")
    add("mc_solve_basket.cp", lambda e: e.lib.hh_mc_solve_basket(e.h, ref(m_()), ref(cfg()), k.ctypes.data,
                                                                 arr(1.0, 0.5).ctypes.data, 2, e.res, NULL),
        INV, "cp must be +1 or -1")
    add("mc_solve_basket.pair", lambda e: e.lib.hh_mc_solve_basket(e.h, ref(m_()), ref(cfg(HEST, EXACT, steps=1)),
                                                                   k.ctypes.data, s.ctypes.data, 2, e.res, NULL),
        UNS, "no simulation method for dynamics 1 with strategy 1")
    # Carr–Madan: more than 1024 sub-panels per lane would be needed (bound/alpha = 196608 itself is accepted)
    add("hh_carr_madan.bound_over_alpha",
        lambda e: e.lib.hh_carr_madan(e.h, ref(m_()), HEST, 0, 0.5, 98304.5, e.host.ctypes.data_as(C.POINTER(C.c_double))),
        INV, CM_BOUND % "hh_carr_madan")
    # Carr–Madan baskets
    for fn, grad in (("hh_carr_madan_basket", False), ("hh_carr_madan_basket_grad", True)):
        def call(e, fn=fn, grad=grad, model=True, dyn=HEST, alpha=1.5, bound=1000.0, **kw):
            g = [e.host.ctypes.data] if grad else []
            return getattr(e.lib, fn)(e.h, ref(m_()) if model else NULL, dyn, 0, alpha, bound, *cm_args(e, **kw),
                                      e.host.ctypes.data, *g)
        add(f"{fn}.null", lambda e, call=call: call(e, model=False), INV, f"{fn}: NULL argument")
        add(f"{fn}.dynamics", lambda e, call=call: call(e, dyn=5), INV, "unknown dynamics 5")
        add(f"{fn}.n_payoffs", lambda e, call=call: call(e, n=0), INV, f"{fn}: 1 .. 2^20 payoffs per call")
        add(f"{fn}.scalars", lambda e, call=call: call(e, alpha=0.0), INV,
            f"{fn}: bad scalars" + (" (Heston: sigma, theta != 0)" if grad else ""))
        add(f"{fn}.bound_over_alpha", lambda e, call=call: call(e, alpha=0.5, bound=98304.5), INV, CM_BOUND % fn)
        add(f"{fn}.payoff_strike", lambda e, call=call: call(e, strikes=(90.0, 100.0, -1.0)), INV,
            f"{fn}: payoff 2: strike, T, discount > 0, cp = +-1")
        add(f"{fn}.payoff_cp", lambda e, call=call: call(e, cps=(1.0, 0.0, 1.0)), INV,
            f"{fn}: payoff 1: strike, T, discount > 0, cp = +-1")
    # LSM on generated paths
    def lsm(e, m=True, c=None, degree=3, disc=0.99, out=True):
        return e.lib.hh_lsm_solve(e.h, ref(m_()) if m else NULL, ref(c or cfg(LOGN, EXACT)), degree, disc,
                                  ref(e.lres) if out else NULL, NULL, NULL, NULL)
    add("lsm_solve.out_null", lambda e: lsm(e, out=False), INV, "hh_lsm_solve: NULL argument")
    add("lsm_solve.pair", lambda e: lsm(e, c=cfg(HEST, EULER)), UNS, LSM_PAIR)
    add("lsm_solve.replay", lambda e: lsm(e, c=cfg(LOGN, EXACT, noise_mode=_ffi.HH_NOISE_REPLAY)), UNS,
        "LSM: GENERATE noise, no dual partials")
    add("lsm_solve.degree0", lambda e: lsm(e, degree=0), INV, LSM_RANGE)
    add("lsm_solve.degree9", lambda e: lsm(e, degree=9), INV, LSM_RANGE)
    add("lsm_solve.n_steps0", lambda e: lsm(e, c=cfg(LOGN, EXACT, steps=0)), INV, LSM_RANGE)
    add("lsm_solve.n_steps_max", lambda e: lsm(e, c=cfg(LOGN, EXACT, steps=65535)), INV,
        "LSM: at most 2^31 - 128 trajectories (x2 antithetic) and 65534 steps")
    add("lsm_solve.discount", lambda e: lsm(e, disc=0.0), INV, "LSM: bad model scalars")
    add("lsm_solve.seeds_null", lambda e: lsm(e, c=cfg(LOGN, EXACT, seeds=None)), INV, "GENERATE needs seeds")
    add("lsm_solve.seeds_len", lambda e: lsm(e, c=cfg(LOGN, EXACT, seeds=SEEDS[:3])), INV,
        "Number of seeds (3) must be >= number of trajectories (10)")
    add("lsm_solve.heston_antithetic", lambda e: lsm(e, c=cfg(HEST, BK, antithetic=1)), UNS,
        "exact Heston grid: GENERATE noise, no dual partials, no antithetic form")
    # LSM on Euler paths, and the Euler grid
    def lsm_e(e, m=True, c=None, state=0, degree=3):
        return e.lib.hh_lsm_solve_euler(e.h, ref(m_()) if m else NULL, ref(c or cfg()), state, degree, 0.99,
                                        ref(e.lres), NULL, NULL, NULL)
    add("lsm_solve_euler.null", lambda e: lsm_e(e, m=False), INV, "hh_lsm_solve_euler: NULL argument")
    add("lsm_solve_euler.degree", lambda e: lsm_e(e, degree=9), INV, LSM_RANGE)
    add("lsm_solve_euler.path_state", lambda e: lsm_e(e, state=2), INV,
        "path_state must be HH_PATH_SPOT (0) or HH_PATH_LOG (1)")
    add("lsm_solve_euler.pair", lambda e: lsm_e(e, c=cfg(LOGN, EXACT)), UNS,
        "Euler grid needs LognormalDynamics or HestonDynamics + EulerMaruyama")
    add("lsm_solve_euler.seeds_len", lambda e: lsm_e(e, c=cfg(seeds=SEEDS[:7])), INV,
        "Number of seeds (7) must be >= number of trajectories (10)")
    def egrid(e, m=True, c=None, state=0, var=False):
        return e.lib.hh_euler_grid(e.h, ref(m_()) if m else NULL, ref(c or cfg()), state, e.host.ctypes.data,
                                   e.host.ctypes.data if var else NULL, 0, e.res)
    add("euler_grid.null", lambda e: egrid(e, m=False), INV, "hh_euler_grid: NULL argument")
    add("euler_grid.path_state", lambda e: egrid(e, state=-1), INV,
        "path_state must be HH_PATH_SPOT (0) or HH_PATH_LOG (1)")
    add("euler_grid.var_lognormal", lambda e: egrid(e, c=cfg(LOGN, EULER), var=True), UNS,
        "Euler grid: variance rows belong to HestonDynamics")
    add("euler_grid.n_steps", lambda e: egrid(e, c=cfg(steps=0)), INV,
        "Euler grid: 1 <= n_paths <= 2^31 - 128, 1 <= n_steps <= 65534")
    # the exact Heston grid
    def hgrid(e, m=True, c=None):
        return e.lib.hh_heston_exact_grid(e.h, ref(m_()) if m else NULL, ref(c or cfg(HEST, BK)), e.host.ctypes.data,
                                          NULL, 0, e.res)
    add("heston_exact_grid.null", lambda e: hgrid(e, m=False), INV, "hh_heston_exact_grid: NULL argument")
    add("heston_exact_grid.pair", lambda e: hgrid(e, c=cfg(HEST, EULER)), UNS,
        "exact Heston grid needs HestonDynamics + HestonBroadieKaya")
    add("heston_exact_grid.n_steps", lambda e: hgrid(e, c=cfg(HEST, BK, steps=0)), INV,
        "exact Heston grid: 1 <= n_paths <= 2^32 - 256, 1 <= n_steps <= 65534")
    add("heston_exact_grid.seeds_null", lambda e: hgrid(e, c=cfg(HEST, BK, seeds=None)), INV, "GENERATE needs seeds")
    # LSM on a caller's grid
    add("lsm_solve_grid.null", lambda e: e.lib.hh_lsm_solve_grid(e.h, ref(m_()), NULL, 10, 4, 3, 0.99, ref(e.lres),
                                                                 NULL, NULL),
        INV, "hh_lsm_solve_grid: NULL argument")
    add("lsm_solve_grid.degree", lambda e: e.lib.hh_lsm_solve_grid(e.h, ref(m_()), e.dev.ptr, 10, 4, 0, 0.99,
                                                                   ref(e.lres), NULL, NULL),
        INV, LSM_RANGE)
    # sharded LSM
    def begin(e, c=None, degree=3, x=True):
        return e.lib.hh_lsm_shard_begin(e.h, ref(m_()), ref(c or cfg(LOGN, EXACT)), degree, 0.99,
                                        e.dev.ptr if x else NULL)
    add("lsm_shard_begin.null", lambda e: begin(e, x=False), INV, "hh_lsm_shard_begin: NULL argument")
    add("lsm_shard_begin.pair", lambda e: begin(e, c=cfg(LOGN, EULER)), UNS, LSM_PAIR)
    add("lsm_shard_begin.degree", lambda e: begin(e, degree=9), INV, LSM_RANGE)
    add("lsm_shard_begin.seeds_len", lambda e: begin(e, c=cfg(LOGN, EXACT, seeds=SEEDS[:2])), INV,
        "Number of seeds (2) must be >= number of trajectories (10)")
    add("lsm_shard_phase.no_begin", lambda e: e.lib.hh_lsm_shard_phase(e.h, _ffi.HH_LSM_PHASE_POW, 0, e.dev.ptr,
                                                                        e.dev.ptr),
        INV, "no sharded LSM in progress")
    add("lsm_shard_finish.no_begin", lambda e: e.lib.hh_lsm_shard_finish(e.h, e.dev.ptr, NULL, NULL, NULL, NULL,
                                                                          NULL),
        INV, "no sharded LSM in progress")
    # staging entry points
    add("replay_pack.null", lambda e: e.lib.hh_replay_pack(e.h, HEST, 10, 4, NULL, 0, e.dev.ptr), INV,
        "hh_replay_pack: bad arguments")
    add("wiener_fill.rho", lambda e: e.lib.hh_wiener_fill(e.h, HEST, 1.5, 1.0, 4, 10, SEEDS.ctypes.data, 0, e.dev.ptr),
        INV, "hh_wiener_fill: bad arguments")
    add("wiener_fill.seeds_null", lambda e: e.lib.hh_wiener_fill(e.h, HEST, 0.5, 1.0, 4, 10, NULL, 0, e.dev.ptr), INV,
        "hh_wiener_fill: bad arguments")
    # multi-GPU
    add("mgpu_solve.null", lambda e: e.lib.hh_mgpu_solve(e.mg1.handle, ref(m_()), ref(cfg()), NULL, NULL), INV,
        "hh_mgpu_solve: NULL argument", "mg1")
    add("mgpu_solve.n_paths", lambda e: e.lib.hh_mgpu_solve(e.mg1.handle, ref(m_()), ref(cfg(n=0)), e.res, NULL), INV,
        "n_paths must be >= 1", "mg1")
    def on_dev():
        c = cfg()
        c.seeds_on_device = 1
        return c
    add("mgpu_solve.on_device", lambda e: e.lib.hh_mgpu_solve(e.mg1.handle, ref(m_()), ref(on_dev()), e.res, NULL),
        INV, "hh_mgpu_solve takes host buffers; device-resident shards go through hh_mgpu_solve_shards", "mg1")
    add("mgpu_solve.seeds_null", lambda e: e.lib.hh_mgpu_solve(e.mg1.handle, ref(m_()), ref(cfg(seeds=None)), e.res,
                                                               NULL),
        INV, "GENERATE needs seeds", "mg1")
    add("mgpu_solve.seeds_len", lambda e: e.lib.hh_mgpu_solve(e.mg2.handle, ref(m_()), ref(cfg(seeds=SEEDS[:5])), e.res,
                                                              NULL),
        INV, "Number of seeds (5) must be >= number of trajectories (10)", "mg2")
    rep = np.zeros(4)
    add("mgpu_solve.replay_len", lambda e: e.lib.hh_mgpu_solve(
        e.mg1.handle, ref(m_()), ref(cfg(LOGN, EXACT, steps=1, seeds=None, noise_mode=_ffi.HH_NOISE_REPLAY,
                                         replay=rep)), e.res, NULL),
        INV, "replay buffer holds 4 elements, 10 needed", "mg1")
    add("mgpu_solve_multi.n_models", lambda e: e.lib.hh_mgpu_solve_multi(e.mg1.handle, two(), 0, ref(cfg()), e.res),
        INV, "hh_mgpu_solve_multi: 1 .. 16 models and their results", "mg1")
    add("mgpu_solve_multi.out_null", lambda e: e.lib.hh_mgpu_solve_multi(e.mg1.handle, two(), 2, ref(cfg()), NULL),
        INV, "hh_mgpu_solve_multi: 1 .. 16 models and their results", "mg1")
    add("mgpu_solve_multi.partials", lambda e: e.lib.hh_mgpu_solve_multi(e.mg1.handle, two(), 2,
                                                                         ref(cfg(n_partials=1)), e.res),
        UNS, "shard 0 (device 0): several models in one pass carry no dual partials (n_partials must be 0)", "mg1")
    add("mgpu_solve_basket.n_payoffs", lambda e: e.lib.hh_mgpu_solve_basket(e.mg1.handle, ref(m_()), ref(cfg()),
                                                                            k.ctypes.data, s.ctypes.data, 0, e.res),
        INV, "hh_mgpu_solve_basket: bad arguments", "mg1")
    add("mgpu_solve_basket.cp", lambda e: e.lib.hh_mgpu_solve_basket(e.mg1.handle, ref(m_()), ref(cfg()),
                                                                     k.ctypes.data, arr(1.0, 2.0).ctypes.data, 2,
                                                                     e.res),
        INV, "shard 0 (device 0): cp must be +1 or -1", "mg1")
    add("mgpu_solve_shards.null", lambda e: e.lib.hh_mgpu_solve_shards(e.mg1.handle, ref(m_()), NULL, e.res, NULL),
        INV, "hh_mgpu_solve_shards: NULL argument", "mg1")
    add("mgpu_solve_shards.empty", lambda e: e.lib.hh_mgpu_solve_shards(e.mg1.handle, ref(m_()), ref(cfg(n=0)), e.res,
                                                                        NULL),
        INV, "every shard is empty", "mg1")
    def mlsm(e, mg="mg2", c=None, degree=3, out=True):
        return e.lib.hh_mgpu_lsm_solve(getattr(e, mg).handle, ref(m_()), ref(c or cfg(LOGN, EXACT)), degree, 0.99,
                                       ref(e.lres) if out else NULL, NULL, NULL)
    add("mgpu_lsm_solve.null", lambda e: mlsm(e, out=False), INV, "hh_mgpu_lsm_solve: NULL argument", "mg2")
    add("mgpu_lsm_solve.replay", lambda e: mlsm(e, c=cfg(LOGN, EXACT, noise_mode=_ffi.HH_NOISE_REPLAY)), INV,
        "hh_mgpu_lsm_solve: GENERATE noise with host seeds", "mg2")
    add("mgpu_lsm_solve.too_few", lambda e: mlsm(e, c=cfg(LOGN, EXACT, n=1, seeds=SEEDS[:1])), INV,
        "every device needs at least one trajectory", "mg2")
    add("mgpu_lsm_solve.seeds_len", lambda e: mlsm(e, c=cfg(LOGN, EXACT, seeds=SEEDS[:4])), INV,
        "Number of seeds (4) must be >= number of trajectories (10)", "mg2")
    add("mgpu_lsm_solve.degree", lambda e: mlsm(e, degree=9), INV, "LSM: 1 <= degree <= 8, n_steps >= 1", "mg2")
    add("mgpu_lsm_solve.one_device", lambda e: mlsm(e, mg="mg1", c=cfg(HEST, EULER)), UNS,
        "device 0: " + LSM_PAIR, "mg1")
    return r


ROWS = rows()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def last_error(e, who):
    if who == "ctx":
        return e.lib.hh_last_error(e.h).decode()
    return e.lib.hh_mgpu_last_error(getattr(e, who).handle).decode()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_argument_error(env, row):
    _, fn, code, text, who = row
    if who == "ctx":  # leave a different text behind first
        env.lib.hh_ctx_set_option(env.h, 999, 0)
    else:
        env.lib.hh_mgpu_set_option(getattr(env, who).handle, 999, 0)
    rc = fn(env)
    assert (rc, last_error(env, who)) == (code, text)


def test_when_the_result_is_zeroed(env):
    """hh_mc_solve zeroes its result before it runs; the multi-model and basket solves only once they have sums."""
    r = env.res
    for i in range(4):
        r[i].price = 7.0
    assert env.lib.hh_mc_solve(env.h, ref(m_()), ref(cfg(seeds=SEEDS[:5])), r, NULL) == INV
    assert r[0].price == 0.0 and r[1].price == 7.0
    r[0].price = 7.0
    models = (_ffi.hh_model * 2)(m_(), _ffi.make_model(S0=101.0))
    assert env.lib.hh_mc_solve_multi(env.h, models, 2, ref(cfg(seeds=SEEDS[:5])), r, NULL) == INV
    k, s = arr(90.0, 110.0), arr(1.0, -1.0)
    assert env.lib.hh_mc_solve_basket(env.h, ref(m_()), ref(cfg(seeds=SEEDS[:5])), k.ctypes.data, s.ctypes.data, 2,
                                      r, NULL) == INV
    assert all(r[i].price == 7.0 for i in range(4))
