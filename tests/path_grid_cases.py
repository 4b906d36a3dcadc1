"""The date rows of the log-spot path family (hh_mc_path_grid) and LSM on them (hh_lsm_solve_path): the sources the tests
run, each with the call that returns the statistics of the same trajectories, and the small helpers both test files share.

A source is one member of the family on a fixed model: its hh_path_source, its hh_model and hh_config for a shape, and its
hh_mc_path_stats* call (the jump form's statistics come back from its solve: it has no statistics-only entry point).
The models are those of the families' own case modules at the identities' shape, 12 steps: jumps at λ·dt ≈ 0.9 (counts
0 … 4 occur), the QE model near the Feller boundary (both branches occur), with and without the martingale correction, a
1 × 64 and a 16 × 128 local-volatility table, Variance Gamma at its base parameters.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Any, Callable

import numpy as np

from hedgehog_jl_amd import _ffi
from tests import bates_cases as bt
from tests import localvol_cases as lc
from tests import merton_cases as mc
from tests import path_payoff_cases as pc
from tests import qe_cases as qc
from tests import vg_cases as vc

GBM, HES = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON
EM, QE, LAW = _ffi.HH_EULER_MARUYAMA, _ffi.HH_QE, _ffi.HH_EXACT_LAW
STEPS = 12
EVERY = (1, 3, 4, 12)
DIVISORS = (1, 2, 3, 4, 6, 12)
SIZES = (1, 63, 64, 65, 257, 513)
H252 = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03)
FLAT = dict(S0=100.0, V0=0.0, kappa=0.0, theta=0.0, sigma=0.25, rho=0.0, r=0.03)


def seeds_for(n, salt=0):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt)


def n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def table(n_t, n_x, sigma=None):
    """an n_t × n_x local-volatility table over log S0 ± 0.6, T = 1: wavy in both directions, or constant at `sigma`"""
    x_lo, h = lc.X0 - 0.6, 1.2 / (n_x - 1)
    times = np.array([0.0]) if n_t == 1 else np.linspace(0.05, 0.95, n_t)
    vols = lc._wavy(n_t, n_x, x_lo, h) if sigma is None else np.full((n_t, n_x), float(sigma))
    assert vols.min() > 0.05
    return dict(times=times, vols=vols, x_lo=x_lo, h=h)


@dataclass
class Source:
    name: str
    kind: int
    dynamics: int
    strategy: int
    model: Callable                  # (T, strike, cp) -> hh_model
    structs: dict                    # field of hh_path_source -> struct
    stats_call: Callable             # (ctx, source, m, c, every, start, stats) -> None
    vanilla_entry: str               # the source's hh_mc_solve_path* entry point
    split: int = 1
    keep: Any = None

    def source(self):
        return _ffi.make_path_source(self.kind, **self.structs)

    def config(self, n, steps, anti=0, seeds=None, **kw):
        return _ffi.make_config(self.dynamics, self.strategy, n, steps, antithetic=anti, em_split=self.split,
                                seeds=seeds_for(n, 17) if seeds is None else seeds, **kw)

    def stats(self, ctx, m, c, every, start):
        """the five statistics of the trajectories of (m, c) over the dates every, 2·every, … (and step 0: start)"""
        out = np.full((_ffi.HH_PATH_STATS, n_total(c)), np.nan)
        self.stats_call(ctx, self, m, c, every, start, out)
        return out

    def vanilla(self, ctx, m, c):
        """the European vanilla of (m.strike, m.cp) through the source's hh_mc_solve_path* on the same trajectories"""
        arr, res = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.VANILLA, m.strike, m.cp)), (_ffi.hh_result * 1)()
        s = self.structs
        extras = [C.byref(s[k]) for k in ("qe", "jump", "localvol", "vg") if k in s]  # the C argument order: qe before jump
        mode = (_ffi.HH_EXTREMES_MONITORED,) if self.kind == _ffi.HH_SOURCE_LOCALVOL else ()
        tail = (None,) if "qe" in s else ()
        ctx.check(getattr(ctx.lib, self.vanilla_entry)(ctx.handle, C.byref(m), *extras, C.byref(c), c.n_steps, 0, *mode, arr, 1,
                                                       res, None, None, *tail))
        return res[0]


def _plain_stats(ctx, src, m, c, every, start, out):
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats(ctx.handle, C.byref(m), C.byref(c), every, start, out.ctypes.data, 0, C.byref(res)))


def _jump_stats(ctx, src, m, c, every, start, out):
    arr, res = (_ffi.hh_path_payoff * 1)(pc.payoff(pc.VANILLA, 100.0, 1.0)), (_ffi.hh_result * 1)()
    ctx.check(ctx.lib.hh_mc_solve_path_jump(ctx.handle, C.byref(m), C.byref(src.structs["jump"]), C.byref(c), every, start,
                                            arr, 1, res, None, out.ctypes.data))


def _qe_stats(ctx, src, m, c, every, start, out):
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_qe(ctx.handle, C.byref(m), C.byref(src.structs["qe"]), C.byref(c), every, start,
                                          out.ctypes.data, 0, None, C.byref(res)))


def _bates_stats(ctx, src, m, c, every, start, out):
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_bates(ctx.handle, C.byref(m), C.byref(src.structs["qe"]), C.byref(src.structs["jump"]),
                                             C.byref(c), every, start, out.ctypes.data, 0, None, C.byref(res)))


def _lv_stats(ctx, src, m, c, every, start, out):
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_lv(ctx.handle, C.byref(m), C.byref(src.structs["localvol"]), C.byref(c), every, start,
                                          _ffi.HH_EXTREMES_MONITORED, out.ctypes.data, 0, C.byref(res)))


def _vg_stats(ctx, src, m, c, every, start, out):
    res = _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_vg(ctx.handle, C.byref(m), C.byref(src.structs["vg"]), C.byref(c), every, start,
                                          out.ctypes.data, 0, C.byref(res)))


def _model(params):
    return lambda T=1.0, strike=100.0, cp=-1.0: _ffi.make_model(**dict(params, T=T, strike=strike, cp=cp))


def _case_params(case):
    """a case dict of the families' modules (r_drift, lam, … beside the model scalars) as make_model's keywords"""
    p = dict(V0=0.0, kappa=0.0, theta=0.0, rho=0.0)
    p.update({k: case[k] for k in ("S0", "V0", "kappa", "theta", "sigma", "rho") if k in case})
    p["r"] = case["r_drift"]
    return p


def euler(name="euler-gbm", dyn=GBM, params=FLAT, split=1):
    return Source(name, _ffi.HH_SOURCE_EULER, dyn, EM, _model(params), {}, _plain_stats, "hh_mc_solve_path", split=split)


def merton(lam=None, sigma=None):
    case = mc.path_case(STEPS, 0)
    if lam is not None:
        case = dict(case, lam=lam)
    if sigma is not None:
        case = dict(case, sigma=sigma)
    return Source("merton" if lam is None else f"merton-lam{lam:g}", _ffi.HH_SOURCE_JUMP, GBM, EM, _model(_case_params(case)),
                  dict(jump=mc.jump_of(case)), _jump_stats, "hh_mc_solve_path_jump")


def qe(mart, case=None, name=None):
    case = case or dict(qc.MODELS["feller"], T=1.0)
    return Source(name or f"qe-mart{mart}", _ffi.HH_SOURCE_QE, HES, QE, _model(_case_params(case)),
                  dict(qe=_ffi.make_qe(0.0, mart)), _qe_stats, "hh_mc_solve_path_qe")


def bates(mart, lam=None, case=None, name=None):
    case = dict(case or dict(qc.MODELS["feller"], T=1.0))
    case.update(lam=bt.PATH_MEAN * STEPS / case["T"] if lam is None else lam, **bt.JUMP)
    return Source(name or (f"bates-mart{mart}" if lam is None else f"bates-mart{mart}-lam{lam:g}"), _ffi.HH_SOURCE_BATES, HES, QE,
                  _model(_case_params(case)), dict(qe=_ffi.make_qe(0.0, mart), jump=bt.jump_struct(case)), _bates_stats,
                  "hh_mc_solve_path_bates")


def localvol(n_t, n_x, sigma=None, r=0.03, name=None):
    surf = table(n_t, n_x, sigma)
    params = dict(FLAT, sigma=float("nan"), r=r)  # model->sigma is not read
    return Source(name or f"localvol-{n_t}x{n_x}" + ("" if sigma is None else "-flat"), _ffi.HH_SOURCE_LOCALVOL, GBM, EM,
                  _model(params), dict(localvol=lc.localvol_of(surf)), _lv_stats, "hh_mc_solve_path_lv", keep=surf)


def vg():
    return Source("vg", _ffi.HH_SOURCE_VG, GBM, LAW, _model(_case_params(vc.BASE)), dict(vg=vc.vg_of(vc.BASE)), _vg_stats,
                  "hh_mc_solve_path_vg")


def identity_sources():
    """every source the bit-for-bit identities run on"""
    return [euler(), euler("euler-heston", HES, H252), euler("euler-heston-unsplit", HES, H252, split=0), merton(),
            qe(0), qe(1), bates(0), bates(1), localvol(1, 64), localvol(16, 128), vg()]


def price_sources():
    """the five new sources at T = 1, r >= 0, on models whose paths stay in ordinary ranges"""
    heston = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r_drift=0.03, T=1.0)
    return [merton(lam=0.8), qe(1, heston, "qe"), bates(1, 0.8, heston, "bates"), localvol(16, 128), vg()]


# ---- the two entry points ------------------------------------------------------------------------------------------------

def path_grid(ctx, src, m, c, every):
    grid = np.full((c.n_steps // every + 1, n_total(c)), np.nan)
    res, source = _ffi.hh_result(), src.source()
    ctx.check(ctx.lib.hh_mc_path_grid(ctx.handle, C.byref(source), C.byref(m), C.byref(c), every, grid.ctypes.data, 0,
                                      C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return grid


def lsm_path(ctx, src, m, c, every, degree, D, want_grid=True, want_stops=True):
    ntot, n_dates = n_total(c), c.n_steps // every
    tau, val = (np.zeros(ntot, dtype=np.int32), np.zeros(ntot)) if want_stops else (None, None)
    grid = np.full((n_dates + 1, ntot), np.nan) if want_grid else None
    res, source = _ffi.hh_lsm_result(), src.source()
    ctx.check(ctx.lib.hh_lsm_solve_path(ctx.handle, C.byref(source), C.byref(m), C.byref(c), every, degree, D, C.byref(res),
                                        tau.ctypes.data if want_stops else None, val.ctypes.data if want_stops else None,
                                        grid.ctypes.data if want_grid else None))
    return res, tau, val, grid
