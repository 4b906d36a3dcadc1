"""The path-statistics kernels swept over model VALUES on the device (tests/path_sweep_cases.py): hh_mc_path_stats_qe /
hh_mc_solve_path_qe, hh_mc_path_stats_bates / hh_mc_solve_path_bates, hh_mc_solve_path_jump, hh_mc_solve_jump and
hh_mc_path_stats_assets / hh_mc_solve_path_assets, hh_mc_path_stats_lv / hh_mc_solve_path_lv (the seven rows under
HH_EXTREMES_BRIDGE, and the five of HH_EXTREMES_MONITORED bit-identical to the first five of those) and
hh_mc_path_stats_ex / hh_mc_solve_path_ex (S_T, CMAX_S and CMIN_S under HH_EXTREMES_BRIDGE on the device's own increments —
the rows path_bridge_cases restates; the other four only finite, positive and bit-identical between the two modes).

Per family one parametrised test over its named cases — the hand-written edge rows on every shape, with and without the
start, with and without mirrors; the drawn models on one shape:
  * PATH BY PATH: every row (and var_T) of every usable member against the family's own 50-digit restatement on the
    draws the device makes itself (the oracle's host Philox, hh_rng.h's formulas; the Merton path form's diffusion
    increments read back from the device), within euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A), imported,
    and never more than 1e-9 of the path's scale (path_sweep_cases.bars).  Two QE rows, kappa_dt_small and sigma_1e-6, are
    ill-conditioned by construction: their 50-digit bars are wider than the values, so what holds the device there is a
    second comparison, with the fp64 restatement of the same formulas, within 1e-9 of scale;
  * TERMINAL LAW: 1, 63 and 65 samples at path_offset 0 and 2³³ − 1; the jump count read off every sample is the exact
    inversion's;
  * PAYOFFS: one hh_mc_solve_path* call per case returns path_values equal to the numpy payoff table on the returned
    statistics, and statistics and var_T bit-identical to the statistics call;
  * FINITENESS: every output of every admitted case is finite, S > 0, var_T >= 0;
  * REJECTIONS: the value just outside every admissibility boundary the edge table touches returns the documented code
    and text without a launch.
tests/test_path_sweep_host.py shows on the CPU that the cases are what they claim and that mutated formulas leave the
bars.  The module prints the worst error/bar per family and row with its case at its end (`-s`)."""
import ctypes as C
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from hedgehog_jl_amd import _ffi  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import merton_cases as mc  # noqa: E402
from tests import path_bridge_cases as bc  # noqa: E402
from tests import path_payoff_cases as pc  # noqa: E402
from tests import path_sweep_cases as sw  # noqa: E402
from tests import qe_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

MONITORED, BRIDGE = _ffi.HH_EXTREMES_MONITORED, _ffi.HH_EXTREMES_BRIDGE
GBM, EXACT, EULER = _ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW, _ffi.HH_EULER_MARUYAMA
ROW_NAMES = ("SUM_S", "SUM_X", "MAX_S", "MIN_S", "S_T", "var_T")
N = sw.N_PATHS
_increments = {}


@pytest.fixture(scope="module")
def worst():
    w = {f: etc.Worst(f"sweep, {f} (device)") for f in sw.FAMILIES}
    yield w
    for f in sw.FAMILIES:
        w[f].report()


# ---- calls -----------------------------------------------------------------------------------------------------------------

def config_of(case, key, anti, n=N):
    fam = case["family"]
    if fam in ("qe", "bates"):
        return qc.config_of(n, key, sw.seeds_of(fam)[:n], anti)
    if fam == "euler":
        return _ffi.make_config(sw.euler_dynamics(case)[0], EULER, n, key, antithetic=anti, em_split=case["em_split"],
                                seeds=sw.seeds_of(fam)[:n])
    if fam in ("merton_path", "assets", "localvol"):
        return _ffi.make_config(GBM, EULER, n, key, antithetic=anti, seeds=sw.seeds_of(fam)[:n])
    return _ffi.make_config(GBM, EXACT, n, 1, antithetic=anti, seeds=np.array([mc.TERMINAL_SEED], dtype=np.uint64), path_offset=key)


def raw_stats(ctx, case, key, every, start, anti, stats, var, extremes=BRIDGE):
    """the statistics entry point of a family that has one -> its return code (extremes: local volatility alone)"""
    m, c = sw.model_struct(case), config_of(case, key, anti)
    sp, vp = (stats.ctypes.data if stats is not None else None), (var.ctypes.data if var is not None else None)
    if case["family"] == "euler":
        return ctx.lib.hh_mc_path_stats_ex(ctx.handle, C.byref(m), C.byref(c), every, start, extremes, sp, 0, None)
    if case["family"] == "localvol":
        lv = sw.localvol_struct(case)
        return ctx.lib.hh_mc_path_stats_lv(ctx.handle, C.byref(m), C.byref(lv), C.byref(c), every, start, extremes, sp, 0, None)
    if case["family"] == "assets":
        a = sw.assets_struct(case)
        return ctx.lib.hh_mc_path_stats_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), every, start, sp, 0, None)
    q = sw.qe_struct(case)
    if case["family"] == "qe":
        return ctx.lib.hh_mc_path_stats_qe(ctx.handle, C.byref(m), C.byref(q), C.byref(c), every, start, sp, 0, vp, None)
    j = sw.jump_struct(case, key)
    return ctx.lib.hh_mc_path_stats_bates(ctx.handle, C.byref(m), C.byref(q), C.byref(j), C.byref(c), every, start, sp, 0, vp, None)


def raw_solve(ctx, case, key, every, start, anti, payoffs, values, stats, var):
    """the solve entry point of a path family -> (its return code, the results)"""
    K = len(payoffs)
    arr, res = (_ffi.hh_path_payoff * K)(*payoffs), (_ffi.hh_result * K)()
    m, c = sw.model_struct(case), config_of(case, key, anti)
    tail = [every, start, arr, K, res] + [a.ctypes.data if a is not None else None for a in (values, stats)]
    fam = case["family"]
    if fam == "euler":
        return ctx.lib.hh_mc_solve_path_ex(ctx.handle, C.byref(m), C.byref(c), every, start, BRIDGE, *tail[2:]), res
    if fam == "localvol":
        lv = sw.localvol_struct(case)
        return ctx.lib.hh_mc_solve_path_lv(ctx.handle, C.byref(m), C.byref(lv), C.byref(c), every, start, BRIDGE, *tail[2:]), res
    if fam == "merton_path":
        j = sw.jump_struct(case, key)
        return ctx.lib.hh_mc_solve_path_jump(ctx.handle, C.byref(m), C.byref(j), C.byref(c), *tail), res
    if fam == "assets":
        a = sw.assets_struct(case)
        return ctx.lib.hh_mc_solve_path_assets(ctx.handle, C.byref(m), C.byref(a), C.byref(c), *tail), res
    tail.append(var.ctypes.data if var is not None else None)
    q = sw.qe_struct(case)
    if fam == "qe":
        return ctx.lib.hh_mc_solve_path_qe(ctx.handle, C.byref(m), C.byref(q), C.byref(c), *tail), res
    j = sw.jump_struct(case, key)
    return ctx.lib.hh_mc_solve_path_bates(ctx.handle, C.byref(m), C.byref(q), C.byref(j), C.byref(c), *tail), res


def raw_terminal(ctx, case, offset, anti, n, term):
    m, c = sw.model_struct(case), config_of(case, offset, anti, n)
    j, res = sw.jump_struct(case, 1), _ffi.hh_result()
    return ctx.lib.hh_mc_solve_jump(ctx.handle, C.byref(m), C.byref(j), C.byref(c), C.byref(res),
                                    term.ctypes.data if term is not None else None), res


def device_rows(ctx, case, key, every, start, anti):
    """-> [rows][n_total]: the five statistics, and var_T where the family has one"""
    total = N * (2 if anti else 1)
    stats = np.full((_ffi.HH_PATH_STATS, total), np.nan)
    if case["family"] in ("localvol", "euler"):
        seven = np.full((_ffi.HH_PATH_STATS_BRIDGE, total), np.nan)
        ctx.check(raw_stats(ctx, case, key, every, start, anti, seven, None, BRIDGE))
        ctx.check(raw_stats(ctx, case, key, every, start, anti, stats, None, MONITORED))
        assert np.array_equal(stats, seven[:_ffi.HH_PATH_STATS]), sw.case_id(case)
        return seven
    if case["family"] == "merton_path":
        rc, _ = raw_solve(ctx, case, key, every, start, anti, [pc.payoff(pc.VANILLA, 100.0, 1.0)], None, stats, None)
        ctx.check(rc)
        return stats
    if case["family"] == "assets":
        ctx.check(raw_stats(ctx, case, key, every, start, anti, stats, None))
        return stats
    var = np.full(total, np.nan)
    ctx.check(raw_stats(ctx, case, key, every, start, anti, stats, var))
    return np.vstack([stats, var[None, :]])


def device_increments(ctx, seeds, n_steps, T, dyn=GBM, rho=0.0, ncomp=1):
    """dW[path][step] (Heston: [path][step][2]): the increments the Euler path kernels draw for these seeds, filled on the
    device"""
    def make():
        buf = _ffi.DeviceBuffer(ctx, 8 * ctx.lib.hh_replay_elems(len(seeds), n_steps, dyn))
        try:
            ctx.check(ctx.lib.hh_wiener_fill(ctx.handle, dyn, rho, T, n_steps, len(seeds), seeds.ctypes.data, 0, buf.ptr))
            ctx.synchronize()
            tiled = buf.download(np.empty(buf.nbytes // 8))
        finally:
            buf.free()
        dW = bc.increments_of(tiled[:n_steps * ncomp * 256], len(seeds), n_steps, ncomp)
        return dW
    k = (n_steps, T, dyn, rho, seeds.tobytes())
    if k not in _increments:
        _increments[k] = make()
    return _increments[k]


def assert_finite(case, got):
    assert np.all(np.isfinite(got)), sw.case_id(case)
    spot_rows = [0] if got.shape[0] == 1 else [pc.SUM_S, pc.MAX_S, pc.MIN_S, pc.S_T] + ([5, 6] if got.shape[0] == 7 else [])
    assert np.all(got[spot_rows] > 0.0), sw.case_id(case)
    if got.shape[0] == 6:
        assert np.all(got[5] >= 0.0), sw.case_id(case)


def compare(worst, case, got, ref, usable, anti, where, n=N):
    """every usable member's rows against the 50-digit reference within sw.bars; on the ILL_CONDITIONED rows, whose 50-digit
    bars hold next to nothing, also against the fp64 restatement within FP64_SIZED of the path's scale -> the misses"""
    bars = sw.bars(case, ref)
    ill = sw.case_id(case) in sw.ILL_CONDITIONED
    near = sw.FP64_SIZED * sw.scales(ref) if ill else None
    bad = []
    for mem in range(2 if anti else 1):
        for i in np.flatnonzero(usable[:n]):
            for row in range(ref["rows"]):
                name = ("S_T", "CMAX_S", "CMIN_S")[row] if ref["rows"] == 3 else \
                    ("CMAX_S", "CMIN_S")[row - 5] if ref["rows"] == 7 and row >= 5 else ROW_NAMES[row if ref["rows"] > 1 else 4]
                here = f"{sw.case_id(case)} {where} anti={anti} member {mem} path {i}"
                bad.append(worst[case["family"]].check(name, got[row][mem * n + i], ref["want"][mem][i][row], bars[mem][i][row], here))
                if ill:
                    bad.append(worst[case["family"]].check(name + " (fp64 restatement)", got[row][mem * n + i],
                                                           mp.mpf(float(ref["f64"][mem][i][row])), near[mem][i][row], here))
    return [b for b in bad if b]


# ---- the path families ---------------------------------------------------------------------------------------------------------

def walked(ctx, oracle, case, key):
    if case["family"] == "merton_path":   # on the device's own diffusion increments
        dW = device_increments(ctx, sw.seeds_of("merton_path"), key, case["model"]["T"])[:, :, 0]
        return sw.cached(("device walk", sw.case_id(case), key), lambda: sw.walk(oracle, case, key, dW=dW))
    if case["family"] == "euler":
        dyn, ncomp = sw.euler_dynamics(case)
        dW = device_increments(ctx, sw.seeds_of("euler"), key, case["model"]["T"], dyn, case["model"]["rho"], ncomp)
        return sw.cached(("device walk", sw.case_id(case), key), lambda: sw.walk(oracle, case, key, dW=dW))
    return sw.walk(oracle, case, key)


def path_family(hhlib, oracle, worst, case):
    bad = []
    for key, every in sw.shapes_of(case):
        w = walked(hhlib, oracle, case, key)
        assert w["counts"]["unusable"] <= sw.CAP
        for start in sw.starts_of(case):
            ref = sw.reference(case, w, every, start)
            for anti in sw.antis_of(case):
                got = device_rows(hhlib, case, key, every, start, anti)
                assert_finite(case, got)
                if case["family"] == "euler":   # the rows the restatement has: S_T, CMAX_S, CMIN_S
                    got = got[[pc.S_T, bc.CMAX_S, bc.CMIN_S]]
                bad += compare(worst, case, got, ref, w["usable"], anti, f"{key}x{every} start={start}")
    assert not bad, "\n".join(bad[:20])
    # the solve form on the case's last shape: the payoff table on its own statistics, the statistics call's bits
    (key, every), start, anti = sw.shapes_of(case)[-1], 1, 1
    payoffs = sw.payoffs_of(case)
    lv = case["family"] in ("localvol", "euler")   # its solve runs under HH_EXTREMES_BRIDGE: seven rows, the payoffs read the bridge's
    n_rows, extremes = (_ffi.HH_PATH_STATS_BRIDGE, BRIDGE) if lv else (_ffi.HH_PATH_STATS, MONITORED)
    values, stats = np.full((len(payoffs), 2 * N), np.nan), np.full((n_rows, 2 * N), np.nan)
    var = np.full(2 * N, np.nan) if case["family"] in ("qe", "bates") else None
    rc, res = raw_solve(hhlib, case, key, every, start, anti, payoffs, values, stats, var)
    hhlib.check(rc)
    again = device_rows(hhlib, case, key, every, start, anti)
    assert np.array_equal(again[:n_rows], stats)
    if var is not None:
        assert np.array_equal(again[5], var)
    assert np.all(np.isfinite(values))
    n_mon = pc.n_mon(key, every, start)
    for k, p in enumerate(payoffs):
        want = bc.payoff_from_stats(stats, p, n_mon, extremes)
        if p.kind == pc.GEOM:
            # numpy's exp against the device's: each within an ulp of G = exp(SUM_X / n), so they differ by 2 ulps of G at
            # the most (4·ε·G leaves a factor 2), and the two rounded differences G − K by that plus half an ulp of the
            # result each.  At G = 100 this is 8.9e-14, within the 1e-13 the families' own tests use at that scale.
            G = np.exp(stats[pc.SUM_X] / float(n_mon))
            assert np.all(np.abs(values[k] - want) <= 4.0 * etc.EPS * G + etc.EPS * np.abs(want)), (sw.case_id(case), k)
        else:
            assert np.array_equal(values[k], want), (sw.case_id(case), k)
        assert res[k].n_paths_done == N and math.isfinite(res[k].price) and math.isfinite(res[k].std_error)


@pytest.mark.parametrize("case", sw.cases("qe"), ids=sw.case_id)
def test_qe(hhlib, oracle, worst, case):
    path_family(hhlib, oracle, worst, case)


@pytest.mark.parametrize("case", sw.cases("bates"), ids=sw.case_id)
def test_bates(hhlib, oracle, worst, case):
    path_family(hhlib, oracle, worst, case)


@pytest.mark.parametrize("case", sw.cases("merton_path"), ids=sw.case_id)
def test_merton_path(hhlib, oracle, worst, case):
    path_family(hhlib, oracle, worst, case)


@pytest.mark.parametrize("case", sw.cases("euler"), ids=sw.case_id)
def test_euler(hhlib, oracle, worst, case):
    path_family(hhlib, oracle, worst, case)


@pytest.mark.parametrize("case", sw.cases("localvol"), ids=sw.case_id)
def test_localvol(hhlib, oracle, worst, case):
    path_family(hhlib, oracle, worst, case)


@pytest.mark.parametrize("case", sw.cases("assets"), ids=sw.case_id)
def test_assets(hhlib, oracle, worst, case):
    path_family(hhlib, oracle, worst, case)


# ---- the terminal law ------------------------------------------------------------------------------------------------------------

def counts_from_samples(S, jm, z, mirror):
    """the jump count each sample was made with: the n in 0 … HH_JUMP_MAX_COUNT whose x_T = m_T ± σ√T·z1 + n·μ_J ± σ_J√n·z2
    is nearest log S — nearest to within rounding, and no other n within 1e-6"""
    sgn = -1.0 if mirror else 1.0
    kbar = math.expm1(jm["mu_j"] + 0.5 * jm["sigma_j"] ** 2)
    mT = math.log(jm["S0"]) + ((jm["r_drift"] - 0.5 * jm["sigma"] ** 2) - jm["lam"] * kbar) * jm["T"]
    n = np.arange(mc.MAX_COUNT + 1, dtype=np.float64)
    out = []
    for s, (z1, z2) in zip(S, z):
        cand = mT + sgn * jm["sigma"] * math.sqrt(jm["T"]) * float(z1) + n * jm["mu_j"] + sgn * jm["sigma_j"] * np.sqrt(n) * float(z2)
        d = np.abs(cand - math.log(s))
        k = int(np.argmin(d))
        assert d[k] < 1e-12 * max(1.0, np.abs(cand).max()) and np.partition(d, 1)[1] > 1e-6, (s, k, np.sort(d)[:2])
        out.append(k)
    return np.array(out)


@pytest.mark.parametrize("case", sw.cases("merton_terminal"), ids=sw.case_id)
def test_merton_terminal(hhlib, oracle, worst, case):
    bad = []
    for offset, _ in sw.shapes_of(case):
        w = sw.walk(oracle, case, offset)
        assert w["counts"]["unusable"] <= sw.CAP
        ref = sw.reference(case, w, 1, 0)
        for anti in (0, 1):
            for n in sw.TERMINAL_SIZES:
                term = np.full(n * (2 if anti else 1), np.nan)
                rc, res = raw_terminal(hhlib, case, offset, anti, n, term)
                hhlib.check(rc)
                assert res.n_paths_done == n
                assert_finite(case, term[None, :])
                bad += compare(worst, case, term[None, :], ref, w["usable"], anti, f"offset {offset} n={n}", n)
                for mem in range(2 if anti else 1):
                    u = np.flatnonzero(w["usable"][:n])
                    got = counts_from_samples(term[mem * n:(mem + 1) * n][u], w["model"], [w["z"][i] for i in u], mem == 1)
                    assert np.array_equal(got, w["N"][u]), (sw.case_id(case), offset, anti, n, mem)
    assert not bad, "\n".join(bad[:20])


# ---- rejections ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", sw.FAMILIES)
def test_the_value_just_outside_every_boundary_is_rejected_without_a_launch(hhlib, family):
    ctx = hhlib
    pay = [pc.payoff(pc.VANILLA, 100.0, 1.0)]
    stats = np.empty((_ffi.HH_PATH_STATS, N))
    names = {"qe": ("hh_mc_path_stats_qe", "hh_mc_solve_path_qe"), "bates": ("hh_mc_path_stats_bates", "hh_mc_solve_path_bates"),
             "merton_path": ("hh_mc_solve_path_jump",), "merton_terminal": ("hh_mc_solve_jump",),
             "assets": ("hh_mc_path_stats_assets", "hh_mc_solve_path_assets"),
             "localvol": ("hh_mc_path_stats_lv", "hh_mc_solve_path_lv"),
             "euler": ("hh_mc_path_stats_ex", "hh_mc_solve_path_ex")}[family]
    stats = np.empty((_ffi.HH_PATH_STATS_BRIDGE, N))
    ctx.enable_timing(True)
    try:
        ctx.read_timings()
        for name, case, n_steps, code, text in sw.rejected(family):
            calls = []
            if family == "merton_terminal":
                calls.append(raw_terminal(ctx, case, 0, 0, N, None)[0])
                calls[0] = (calls[0], ctx.lib.hh_last_error(ctx.handle).decode())
            else:
                if family != "merton_path":
                    calls.append((raw_stats(ctx, case, n_steps, 1, 0, 0, stats, None), ctx.lib.hh_last_error(ctx.handle).decode()))
                calls.append((raw_solve(ctx, case, n_steps, 1, 0, 0, pay, None, None, None)[0], ctx.lib.hh_last_error(ctx.handle).decode()))
            for who, (rc, msg) in zip(names, calls):
                assert rc == code and text in msg and who in msg, (name, who, rc, code, text, msg)
        assert ctx.read_timings() == []   # nothing was launched
    finally:
        ctx.enable_timing(False)
