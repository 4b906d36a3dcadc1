"""The device's Euler–Maruyama kernels with their forward-mode Greeks (hh_sim.h: the fused per-step map of
HestonModel::step, its two clip flags, the reciprocal + Newton step, sqrt_clipped; hh_kernels.hip: the carried basis
derivatives and the assembly of the requested directions from them and from the two in-the-money sums) against the
scheme's step-by-step dual rules in mpmath at 50 digits (oracle/euler_exact.py), PATH BY PATH, on the cases of
tests/golden/euler_tangent_exact.json: S_T, the price contribution and all eight partials of every usable path, sums over
all paths, assembled directions, GENERATE on live increments and the basket.  The bars are tests/euler_tangent_cases.py's:
20·max(e64, ε·A) per path and slot, nothing taken from the device or the C oracle.  The module prints its worst
error/bar per kind of comparison at its end (`-s`)."""
import ctypes as C

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from hedgehog_jl_amd import _ffi  # noqa: E402
from oracle import euler_exact as ex  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests.euler_tangent_cases import BY_ID, IDS, NS, SLOTS  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = [pytest.param(False, id="tile-major"), pytest.param(True, id="path-major")]


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("euler_tangent_exact (device)")
    yield w
    w.report()


def solve(ctx, m, c):
    res = _ffi.hh_result()
    term = np.zeros(c.n_paths * (2 if c.antithetic else 1))
    ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(m), C.byref(c), C.byref(res), term.ctypes.data))
    return res, term


def usable_paths(ref, j):
    return [int(i) for i in np.flatnonzero(ref["payoffs"][j]["usable"])]


# ---- (a) one path per solve ----------------------------------------------------------------------------------

@pytest.mark.parametrize("path_major", LAYOUTS)
@pytest.mark.parametrize("name", IDS)
def test_one_path_per_solve(hhlib, worst, name, path_major):
    """n_paths = 1, eight unit seeds: dprice[k] is that path's discounted partial; tile-major (lane 0 of one tile) and
    path-major REPLAY."""
    case = BY_ID[name]
    ref = etc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        m = etc.model_of(case, strike, cp)
        for i in usable_paths(ref, j):
            res, term = solve(hhlib, m, etc.config_of(case, [i], path_major))
            assert res.n_paths_done == 1
            bad += etc.check_solve(worst, case, ref, j, [i], res, term, "device")
    assert not bad, "\n".join(bad[:20])


# ---- (b) all paths in one solve ------------------------------------------------------------------------------

@pytest.mark.parametrize("path_major", LAYOUTS)
@pytest.mark.parametrize("name", IDS)
def test_all_paths_in_one_solve(hhlib, worst, name, path_major):
    """Lanes 0…31 mix in- and out-of-the-money paths: the two in-the-money sums and the closed-form finish of the spot,
    rate and strike directions matter.  Every terminal to its per-path bar, price and dprice[0..7] to the sum bar."""
    case = BY_ID[name]
    ref = etc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        paths = usable_paths(ref, j)
        res, term = solve(hhlib, etc.model_of(case, strike, cp), etc.config_of(case, paths, path_major))
        assert res.n_paths_done == len(paths)
        bad += etc.check_solve(worst, case, ref, j, paths, res, term, "device")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name", ["H252-s50-split", "FV-s16-classic-anti", "kdt-s7-split", "GBM-sigma0.2-s7"])
def test_both_record_reductions(hhlib, worst, name, fuse):
    """The requested directions are assembled where the records are added: by reduce_records_kernel
    (HH_OPT_FUSE_REDUCE = 0) or inside the simulation kernel (1; the default picks by size)."""
    case = BY_ID[name]
    ref = etc.reference(case)
    bad = []
    hhlib.set_option(_ffi.HH_OPT_FUSE_REDUCE, fuse)
    try:
        for j, (strike, cp) in enumerate(case["payoff_list"]):
            paths = usable_paths(ref, j)
            res, term = solve(hhlib, etc.model_of(case, strike, cp), etc.config_of(case, paths))
            bad += etc.check_solve(worst, case, ref, j, paths, res, term, f"device fuse={fuse}")
    finally:
        hhlib.set_option(_ffi.HH_OPT_FUSE_REDUCE, 2)
    assert not bad, "\n".join(bad[:20])


# ---- (c) assembly --------------------------------------------------------------------------------------------

def _mixed(D):
    """the seven directions of test_gpu_parity.py::test_mixed_active_and_passive_directions"""
    return {"S0": [1, 0, 0, 0, 0.5, 0, 0], "V0": [0, 1, 0, 0, 0.25, 0, 0], "r_drift": [0, 0, 1, 0, 0, 0.1, 0],
            "discount": [0, 0, -D, 0, 0, -0.1 * D, 0], "strike": [0, 0, 0, 1, 0, 0.3, 0],
            "sigma": [0, 0, 0, 0, 0, 0, 1], "kappa": [0, 0, 0, 0, 0.1, 0, 0]}


DIRECTIONS = {
    "mixed": _mixed,
    "sigma-only": lambda D: {"sigma": [1]},
    "theta-then-kappa": lambda D: {"theta": [1, 0], "kappa": [0, 1]},
    "V0-passive-sigma": lambda D: {"V0": [1, 0, 0], "S0": [0, 1, 0], "sigma": [0, 0, 1]},
    "five": lambda D: {"sigma": [1, 0, 0, 0, 0], "strike": [0, 1, 0, 0, 0], "kappa": [0, 0, 1, 0, 0],
                       "r_drift": [0, 0, 0, 1, 0], "V0": [0, 0, 0, 0, 1]},
    "strike-and-discount": lambda D: {"strike": [1, 0.5], "discount": [0.25, 1]},
}


@pytest.mark.parametrize("which", list(DIRECTIONS))
@pytest.mark.parametrize("name", ["H252-s16-split", "H252-s16-classic", "FV-s16-split", "FV-s16-classic-anti"])
def test_assembled_directions(hhlib, worst, name, which):
    """Directions mixing carried (V0, κ, θ, σ) and passive (spot, rate, strike, discount) seeds, and seed sets that
    change which carried slot holds which parameter, against linear combinations of the reference Jacobian."""
    case = BY_ID[name]
    ref = etc.reference(case)
    seeds = DIRECTIONS[which](case["discount"])
    P = len(next(iter(seeds.values())))
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        pj, paths = ref["payoffs"][j], usable_paths(ref, j)
        n = len(paths)
        m = etc.model_of(case, strike, cp, seeds=seeds, n_partials=P)
        res, _ = solve(hhlib, m, etc.config_of(case, paths, n_partials=P))
        price, bar = etc.sum_of(pj["price"], pj["price_e64"], pj["price_A"], paths, int(case["antithetic"]))
        for k in range(P):
            direction = [seeds.get(slot, [0.0] * P)[k] for slot in SLOTS]
            want, dbar = etc.assembled(direction, price, bar)
            with mp.workdps(ex.DPS):
                want = want / n
            bad.append(worst.check("assembled direction", res.dprice[k], want, dbar / n,
                                   f"{name} K={strike:g} cp={cp:+.0f} {which}[{k}]"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ---- (d) GENERATE --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("tag", ["H252", "FV", "kdt"])
def test_generate_on_live_increments(hhlib, worst, tag, split):
    """The P > 0 GENERATE instantiations of euler_kernel: increments of 32 seeds filled on the device
    (hh_wiener_fill), copied to the host, the reference evaluated on them live; the GENERATE solve of those seeds is
    held to the sum bars — after its terminals are shown to equal, bit for bit, REPLAY's on the filled increments
    (the kernel's draw and wiener_fill_kernel use the same normal_pair and the same forms).  H252 and FV keep all 32
    paths; kdt leaves out 4 (split) and 1 (classic) whose comparisons fall under the guard."""
    import torch
    base = next(c for c in etc.CASES if c["tag"] == tag)
    n, steps = 32, 16
    seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(len(tag) + 2 * split)
    buf = torch.zeros(hhlib.lib.hh_replay_elems(n, steps, etc.HES), dtype=torch.float64, device="cuda")
    hhlib.check(hhlib.lib.hh_wiener_fill(hhlib.handle, etc.HES, base["rho"], base["T"], steps, n, seeds.ctypes.data, 0,
                                         buf.data_ptr()))
    hhlib.synchronize()
    tiled = buf.cpu().numpy()
    case = dict(base)
    case.update(id=f"{tag}-generate-{'split' if split else 'classic'}", n_steps=steps, em_split=split, antithetic=0,
                payoff_list=[(base["S0"], 1.0), (base["S0"], -1.0)],
                dW=np.ascontiguousarray(tiled.reshape(steps, 2, 256).transpose(2, 0, 1)[:n]))
    ref = ex.reference(case, case["payoff_list"])
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        m = etc.model_of(case, strike, cp)
        # H252 and FV: the generator's floor.  kdt: κ·dt = 2.5 over 16 steps lets the magnitude of v outgrow v by
        # 3.5/1.5 per step, so more comparisons fall under the 2⁻³⁰ guard there; those paths are left out, as
        # everywhere, and at least half must remain
        paths = usable_paths(ref, j)
        print(f"\n{case['id']} K={strike:g} cp={cp:+.0f}: {n - len(paths)} of {n} paths left out")
        assert n - len(paths) <= (n // 2 if tag == "kdt" else etc.MAX_UNUSABLE * n)
        gen = _ffi.make_config(etc.HES, _ffi.HH_EULER_MARUYAMA, len(paths), steps, em_split=split,
                               seeds=seeds[paths], n_partials=NS)
        rg, tg = solve(hhlib, m, gen)
        rr, tr = solve(hhlib, m, etc.config_of(case, paths))
        np.testing.assert_array_equal(tg, tr)
        bad += etc.check_solve(worst, case, ref, j, paths, rg, tg, "device GENERATE")
        bad += etc.check_solve(worst, case, ref, j, paths, rr, tr, "device REPLAY of the filled increments")
    assert not bad, "\n".join(bad[:20])


# ---- (e) basket ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["H252-s16-split-anti", "FV-s16-split", "kdt-s7-classic"])
def test_basket(hhlib, worst, name):
    """hh_mc_solve_basket: three strikes, both signs, one simulation; each payoff's price and partials against the
    reference evaluated at that strike (strike partials are not carried through a basket)."""
    case = dict(BY_ID[name])
    S0 = case["S0"]
    case.update(id=name + "-basket", payoff_list=[(K, cp) for cp in (1.0, -1.0) for K in (S0 / 2, S0, 3 * S0)])
    ref = ex.reference(case, case["payoff_list"])
    ok = np.all([pj["usable"] for pj in ref["payoffs"]], axis=0)
    paths = [int(i) for i in np.flatnonzero(ok)]
    assert len(paths) >= ref["n"] - 1
    strikes = np.array([K for K, _ in case["payoff_list"]])
    cps = np.array([cp for _, cp in case["payoff_list"]])
    seeds = {slot: [1.0 if q == k else 0.0 for q in range(NS - 1)] for k, slot in enumerate(SLOTS[:-1])}
    m = etc.model_of(case, S0, 1.0, seeds=seeds, n_partials=NS - 1)  # a strike seed is refused by the basket
    c = etc.config_of(case, paths, n_partials=NS - 1)
    res = (_ffi.hh_result * len(strikes))()
    term = np.zeros(len(paths) * ref["members"])
    hhlib.check(hhlib.lib.hh_mc_solve_basket(hhlib.handle, C.byref(m), C.byref(c), strikes.ctypes.data, cps.ctypes.data,
                                             len(strikes), res, term.ctypes.data))
    bad = []
    for j in range(len(strikes)):
        bad += etc.check_solve(worst, case, ref, j, paths, res[j], term if j == 0 else None, "device basket",
                               skip=("strike",))
    assert not bad, "\n".join(bad[:20])
