"""The path-statistics family — path_stats_kernel (monitored and bridge), jump_stats_kernel, qe_stats_kernel,
bates_stats_kernel, assets_stats_kernel — pinned BIT FOR BIT: what tests/golden/make_path_family_pins.py records and
tests/test_gpu_path_family_pins.py recomputes.

Every statistics case is one hh_mc_path_stats* call on 257 trajectories (two workgroups, the last with one live lane);
its pin is the SHA-256 of the returned statistics' bytes and, where the entry point has one, of var_T's.  The shapes:
6 and 7 steps (7 half-reads the Philox block that feeds two steps), every monitor_every of 1, 2, 3, n_steps that divides
n_steps, include_start 0 and 1, antithetic 0 and 1.  Models and seeds are those of the families' own case modules,
chosen there so that both QE branches and jumps occur at these sizes; `seen` restates that on the CPU for the shapes
used here.  One hh_mc_solve_path* call per family with four payoffs pins the bytes of the prices and standard errors.
"""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

from hedgehog_jl_amd import _ffi
from tests import assets_cases as ac
from tests import bates_cases as bt
from tests import merton_cases as mc
from tests import path_bridge_cases as bc
from tests import path_payoff_cases as pc
from tests import qe_cases as qc
from tests import test_gpu_path_payoff as base

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_family_pins.json")
N = 257
SHAPES = [(steps, every) for steps in (6, 7) for every in (1, 2, 3, steps) if steps % every == 0]
ASSET_SHAPES = [(6, 1), (6, 3)]
FLAGS = [(start, anti) for start in (0, 1) for anti in (0, 1)]


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


def toolchain():
    """the compiler's own version string: a pin holds for the toolchain that built the library it was recorded on"""
    return subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.strip()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _n_total(c):
    return int(c.n_paths) * (2 if c.antithetic else 1)


def _stats(ctx, entry, rows, c, every, start, *structs, var=False):
    """entry(ctx, structs…, c, every, start, stats, 0, [var_T,] out) -> {"stats": sha, ["var_T": sha]}"""
    stats, res = np.empty((rows, _n_total(c))), _ffi.hh_result()
    tail = [stats.ctypes.data, 0]
    vt = np.empty(_n_total(c)) if var else None
    if var:
        tail.append(vt.ctypes.data)
    ctx.check(entry(ctx.handle, *[C.byref(s) for s in structs], C.byref(c), every, start, *tail, C.byref(res)))
    assert res.n_paths_done == c.n_paths
    return dict(stats=sha(stats), var_T=sha(vt)) if var else dict(stats=sha(stats))


def _stats_ex(ctx, m, c, every, start, extremes):
    stats, res = np.empty((bc.ROWS[extremes], _n_total(c))), _ffi.hh_result()
    ctx.check(ctx.lib.hh_mc_path_stats_ex(ctx.handle, C.byref(m), C.byref(c), every, start, extremes, stats.ctypes.data, 0,
                                          C.byref(res)))
    return dict(stats=sha(stats))


def _solve(ctx, entry, payoffs, head, tail):
    """entry(ctx, *head, payoffs, K, out, *tail) -> the bytes of (price, std_error) of every payoff"""
    K = len(payoffs)
    arr, res = (_ffi.hh_path_payoff * K)(*payoffs), (_ffi.hh_result * K)()
    ctx.check(entry(ctx.handle, *head, arr, K, res, *tail))
    out = np.array([[r.price, r.std_error] for r in res])
    assert np.all(np.isfinite(out)) and np.all(out[:, 1] > 0.0)
    return dict(result=sha(out))


def stat_cases():
    """-> (id, run(ctx) -> dict of digests) of every statistics case, in a fixed order"""
    em_seeds = base.seeds_for(N)
    for name, (dyn, split, params) in base.MODELS.items():
        for form, ext in (("monitored", bc.MONITORED), ("bridge", bc.BRIDGE)):
            for steps, every in SHAPES:
                for start, anti in FLAGS:
                    def run(ctx, a=(dyn, split, params, ext, steps, every, start, anti)):
                        dyn, split, params, ext, steps, every, start, anti = a
                        c = _ffi.make_config(dyn, base.EULER, N, steps, antithetic=anti, em_split=split, seeds=em_seeds)
                        return _stats_ex(ctx, _ffi.make_model(**params), c, every, start, ext)
                    yield f"em/{name}/{form}/{steps}x{every}/start{start}/anti{anti}", run
    for steps, every in SHAPES:
        for start, anti in FLAGS:
            def run(ctx, a=(steps, every, start, anti)):
                steps, every, start, anti = a
                case = mc.path_case(steps, anti)
                c = _ffi.make_config(mc.GBM, mc.EULER, N, steps, antithetic=anti, seeds=mc.path_seeds())
                # the statistics of the jump form come back from its solve (it has no statistics-only entry point)
                K = 1
                arr, res = (_ffi.hh_path_payoff * K)(pc.payoff(pc.VANILLA, 100.0, 1.0)), (_ffi.hh_result * K)()
                stats = np.empty((_ffi.HH_PATH_STATS, _n_total(c)))
                ctx.check(ctx.lib.hh_mc_solve_path_jump(ctx.handle, C.byref(mc.model_of(case)), C.byref(mc.jump_of(case)),
                                                        C.byref(c), every, start, arr, K, res, None, stats.ctypes.data))
                return dict(stats=sha(stats))
            yield f"merton/{steps}x{every}/start{start}/anti{anti}", run
    for fam in ("qe", "bates"):
        for name in qc.MODELS:
            for mart in (0, 1):
                for steps, every in SHAPES:
                    for start, anti in FLAGS:
                        def run(ctx, a=(fam, name, mart, steps, every, start, anti)):
                            fam, name, mart, steps, every, start, anti = a
                            q = _ffi.make_qe(0.0, mart)
                            if fam == "qe":
                                c = qc.config_of(N, steps, qc.path_seeds(), anti)
                                return _stats(ctx, ctx.lib.hh_mc_path_stats_qe, _ffi.HH_PATH_STATS, c, every, start,
                                              qc.model_of(qc.MODELS[name]), q, var=True)
                            case = bt.path_case(name, steps)
                            c = bt.config_of(N, steps, bt.path_seeds(), anti)
                            return _stats(ctx, ctx.lib.hh_mc_path_stats_bates, _ffi.HH_PATH_STATS, c, every, start,
                                          bt.model_of(case), q, bt.jump_struct(case), var=True)
                        yield f"{fam}/{name}/mart{mart}/{steps}x{every}/start{start}/anti{anti}", run
    for d in range(1, ac.MAX + 1):
        for kind in ac.KINDS:
            for steps, every in ASSET_SHAPES:
                for start, anti in FLAGS:
                    def run(ctx, a=(d, kind, steps, every, start, anti)):
                        d, kind, steps, every, start, anti = a
                        case = ac.path_case(d)
                        c = _ffi.make_config(ac.GBM, ac.EULER, N, steps, antithetic=anti, seeds=ac.path_seeds())
                        return _stats(ctx, ctx.lib.hh_mc_path_stats_assets, _ffi.HH_PATH_STATS, c, every, start,
                                      ac.model_of(case), ac.assets_of(case, kind))
                    yield f"assets/d{d}/kind{kind}/{steps}x{every}/start{start}/anti{anti}", run


def solve_cases():
    """one hh_mc_solve_path* call per family: four payoffs, 7 steps, antithetic, the start included"""
    four = mc.payoff_list()[:4]  # vanilla, arithmetic and geometric Asian, barrier
    steps, every, start, anti = 7, 1, 1, 1
    ref = C.byref

    def em(ctx, bridge):
        dyn, split, params = base.MODELS["heston-classic-clipped"]
        c = _ffi.make_config(dyn, base.EULER, N, steps, antithetic=anti, em_split=split, seeds=base.seeds_for(N))
        m = _ffi.make_model(**params)
        if bridge:
            return _solve(ctx, ctx.lib.hh_mc_solve_path_ex, four, (ref(m), ref(c), every, start, bc.BRIDGE), (None, None))
        return _solve(ctx, ctx.lib.hh_mc_solve_path, four, (ref(m), ref(c), every, start), (None, None))

    def merton(ctx):
        case = mc.path_case(steps, anti)
        c = _ffi.make_config(mc.GBM, mc.EULER, N, steps, antithetic=anti, seeds=mc.path_seeds())
        return _solve(ctx, ctx.lib.hh_mc_solve_path_jump, four, (ref(mc.model_of(case)), ref(mc.jump_of(case)), ref(c), every, start),
                      (None, None))

    def qe(ctx):
        c = qc.config_of(N, steps, qc.path_seeds(), anti)
        return _solve(ctx, ctx.lib.hh_mc_solve_path_qe, four,
                      (ref(qc.model_of(qc.MODELS["feller"])), ref(_ffi.make_qe(0.0, 1)), ref(c), every, start), (None, None, None))

    def bates(ctx):
        case = bt.path_case("feller", steps)
        c = bt.config_of(N, steps, bt.path_seeds(), anti)
        return _solve(ctx, ctx.lib.hh_mc_solve_path_bates, four,
                      (ref(bt.model_of(case)), ref(_ffi.make_qe(0.0, 1)), ref(bt.jump_struct(case)), ref(c), every, start),
                      (None, None, None))

    def assets(ctx):
        case = ac.path_case(3)
        c = _ffi.make_config(ac.GBM, ac.EULER, N, 6, antithetic=anti, seeds=ac.path_seeds())
        return _solve(ctx, ctx.lib.hh_mc_solve_path_assets, ac.payoff_list(case, ac.SUM)[:4],
                      (ref(ac.model_of(case)), ref(ac.assets_of(case, ac.SUM)), ref(c), 3, start), (None, None))

    yield "solve/em", lambda ctx: em(ctx, False)
    yield "solve/em-bridge", lambda ctx: em(ctx, True)
    yield "solve/merton", merton
    yield "solve/qe", qe
    yield "solve/bates", bates
    yield "solve/assets", assets


def compute(ctx):
    """every case's digests, computed on the device through the C-ABI"""
    return {cid: run(ctx) for cases in (stat_cases(), solve_cases()) for cid, run in cases}


# ---- what the cases exercise, restated on the CPU ------------------------------------------------------------------------

def seen(oracle):
    """For the shapes used here: the QE branches the fp64 restatement takes (qe_cases.walk / bates_cases.walk; a state's
    branch does not depend on the martingale correction) and the jump counts the fp64 inversion gives
    (merton_cases.poisson_fp64) — per family, model and step count, over both members of all 257 trajectories."""
    out = {}
    for steps in (6, 7):
        U = mc.path_uniforms(oracle, mc.path_seeds(), steps)
        mean = mc.path_mean(mc.path_case(steps, 0))
        counts = np.bincount([mc.poisson_fp64(float(u), mean) for u in U.ravel()])
        out[f"merton/{steps}"] = dict(N=counts.tolist())
        Zq, Uq = qc.step_normals(oracle, qc.path_seeds(), steps), qc.step_uniforms(oracle, qc.path_seeds(), steps)
        d = bt.draws(oracle, bt.path_seeds(), steps)
        for name in qc.MODELS:
            rec = []
            for i in range(N):
                Z64 = [(float(a), float(b)) for a, b in Zq[i]]
                for mirror in (False, True):
                    qc.walk(qc.MODELS[name], steps, float, Z64, Uq[i], mirror, 0, rec)
            out[f"qe/{name}/{steps}"] = dict(quadratic=sum(1 for r in rec if r[1]), exponential=sum(1 for r in rec if not r[1]))
            case = bt.path_case(name, steps)
            Nb = bt.counts(d["UJ"], bt.path_mean(case, steps), check=False)
            rec = []
            for i in range(N):
                d64 = bt._float_draws(d, i)
                for mirror in (False, True):
                    bt.walk(case, steps, float, d64, i, Nb[i], mirror, 0, rec)
            out[f"bates/{name}/{steps}"] = dict(quadratic=sum(1 for r in rec if r[1]), exponential=sum(1 for r in rec if not r[1]),
                                                N=np.bincount(Nb.ravel()).tolist())
    return out


def check_seen(s):
    """every QE and Bates case takes both branches, every jump case has trajectories with one and with several jumps"""
    for key, rec in s.items():
        if "quadratic" in rec:
            assert rec["quadratic"] > 0 and rec["exponential"] > 0, (key, rec)
        if "N" in rec:
            assert len(rec["N"]) >= 3 and all(n > 0 for n in rec["N"][:3]), (key, rec)
