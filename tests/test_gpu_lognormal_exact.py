"""The device's closed-form lognormal kernels — exact_gbm_kernel (hh_kernels.hip) in its 4-, 8- and 64-pair lane forms
with its forward-mode Greeks and the closed-form finish of the passive directions, and gbm_grid_kernel (hh_lsm.hip), the
path source of hh_lsm_solve, with its exp(2a)·rcp(e) mirror — against the reference's formulas in mpmath at 50 digits
(oracle/lognormal_exact.py), PATH BY PATH, on the cases of tests/golden/lognormal_exact.json.  The bars are
tests/euler_tangent_cases.py's: 20·max(e64, ε·A) per path and slot, nothing taken from the device or the C oracle.
Whole ensembles (ragged shapes of the 4-pair form, the 8-pair form) are held to a vectorised long-double evaluation at
the same rule without e64; sums to math.fsum of the payoffs of the device's own terminals.  The module prints its worst
error/bar per kind of comparison at its end (`-s`)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from hedgehog_jl_amd import _ffi  # noqa: E402
from oracle import lognormal_exact as lx  # noqa: E402
from tests import euler_tangent_cases as etc  # noqa: E402
from tests import lognormal_exact_cases as lc  # noqa: E402
from tests.lognormal_exact_cases import BY_ID, EXACT, GBM, IDS, NS, SLOTS  # noqa: E402
from tests.test_gpu_euler_tangent_exact import DIRECTIONS  # noqa: E402
from tests.test_gpu_rng_device import PAIR_BAR  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = etc.EPS
LD = np.longdouble
WG = 512  # trajectories of one workgroup per pair index jp: lane tid holds jp·512 + 2·tid, + 1
N8 = 2048 * 512 * 8 + 700
N64 = 2048 * 512 * 64 + 513


@pytest.fixture(scope="module")
def worst():
    w = etc.Worst("lognormal_exact (device)")
    yield w
    w.report()


def solve(ctx, m, c, want_terminal=True):
    res = _ffi.hh_result()
    term = np.zeros(c.n_paths * (2 if c.antithetic else 1)) if want_terminal else None
    ctx.check(ctx.lib.hh_mc_solve(ctx.handle, C.byref(m), C.byref(c), C.byref(res), term.ctypes.data if want_terminal else None))
    return res, term


def zero_columns(res, where):
    return [f"{where}: d/d{slot} = {res.dprice[SLOTS.index(slot)]!r}, not 0.0" for slot in lc.ZERO_SLOTS
            if res.dprice[SLOTS.index(slot)] != 0.0]


def note(worst, kind, ratio, where):
    if ratio > worst.w.get(kind, (-1.0, ""))[0]:
        worst.w[kind] = (float(ratio), where)


# ---- (a) one path per solve ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IDS)
def test_one_path_per_solve(hhlib, worst, name):
    """REPLAY, n_paths = 1, eight unit seeds: S_T, the price and dprice[0..7] of every usable path against its bar;
    the V0, κ, θ columns are exact zeros."""
    case = BY_ID[name]
    ref = lc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        m = lc.model_of(case, strike, cp)
        for i in lc.usable_paths(ref, j):
            res, term = solve(hhlib, m, lc.config_of(case, [i]))
            assert res.n_paths_done == 1
            bad += etc.check_solve(worst, case, ref, j, [i], res, term, "device")
            bad += zero_columns(res, f"{name} path {i}")
    assert not bad, "\n".join(bad[:20])


# ---- (b) all paths in one solve --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 32])
@pytest.mark.parametrize("name", IDS)
def test_all_paths_in_one_solve(hhlib, worst, name, n):
    """The first 2, 3 or 32 paths of a case in one solve: two reach slot j = 1 of lane 0's pair, three reach lane 1.
    Every terminal — the mirrors' at terminal[n + i] — against its path bar, price and dprice against the sum bar."""
    case = BY_ID[name]
    ref = lc.reference(case)
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        paths = list(range(n))
        assert set(paths) <= set(lc.usable_paths(ref, j))
        res, term = solve(hhlib, lc.model_of(case, strike, cp), lc.config_of(case, paths))
        assert res.n_paths_done == n
        bad += etc.check_solve(worst, case, ref, j, paths, res, term, "device")
        bad += zero_columns(res, f"{name} n={n}")
    assert not bad, "\n".join(bad[:20])


# ---- (c) both record reductions --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name", ["ref-anti", "bench", "bench-compat-anti", "tiny-sigma-anti", "short-compat"])
def test_both_record_reductions(hhlib, worst, name, fuse):
    """The passive directions (spot, rate, strike) are finished where the records are added: by reduce_records_kernel
    (HH_OPT_FUSE_REDUCE = 0) or inside the simulation kernel (1; the default picks by size)."""
    case = BY_ID[name]
    ref = lc.reference(case)
    bad = []
    hhlib.set_option(_ffi.HH_OPT_FUSE_REDUCE, fuse)
    try:
        for j, (strike, cp) in enumerate(case["payoff_list"]):
            paths = lc.usable_paths(ref, j)
            res, term = solve(hhlib, lc.model_of(case, strike, cp), lc.config_of(case, paths))
            bad += etc.check_solve(worst, case, ref, j, paths, res, term, f"device fuse={fuse}")
    finally:
        hhlib.set_option(_ffi.HH_OPT_FUSE_REDUCE, 2)
    assert not bad, "\n".join(bad[:20])


# ---- (d) assembled directions ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(DIRECTIONS))
@pytest.mark.parametrize("name", ["ref", "ref-compat-anti", "bench-anti", "short-compat"])
def test_assembled_directions(hhlib, worst, name, which):
    """The directions of tests/test_gpu_euler_tangent_exact.py, restricted to the slots this law reads (seeds on V0, κ,
    θ dropped; a direction left without a seed must come out an exact zero), against linear combinations of the
    reference Jacobian: σ is carried per path, spot, rate, strike and discount are finished in closed form."""
    case = BY_ID[name]
    ref = lc.reference(case)
    full = DIRECTIONS[which](case["discount"])
    P = len(next(iter(full.values())))
    seeds = {slot: v for slot, v in full.items() if slot not in lc.ZERO_SLOTS}
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        pj, paths = ref["payoffs"][j], lc.usable_paths(ref, j)
        n = len(paths)
        res, _ = solve(hhlib, lc.model_of(case, strike, cp, seeds=seeds, n_partials=P), lc.config_of(case, paths, n_partials=P))
        price, bar = etc.sum_of(pj["price"], pj["price_e64"], pj["price_A"], paths, int(case["antithetic"]))
        for k in range(P):
            direction = [seeds.get(slot, [0.0] * P)[k] for slot in SLOTS]
            want, dbar = etc.assembled(direction, price, bar)
            with mp.workdps(lx.DPS):
                want = want / n
            bad.append(worst.check("assembled direction", res.dprice[k], want, dbar / n,
                                   f"{name} K={strike:g} cp={cp:+.0f} {which}[{k}]"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ---- (e) basket ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ref-anti", "bench-compat", "scale-large-anti"])
def test_basket(hhlib, worst, name):
    """hh_mc_solve_basket: three strikes, both signs, one simulation; each payoff's price and partials against the
    reference evaluated at that strike (strike partials are not carried through a basket)."""
    case = dict(BY_ID[name])
    S0 = case["S0"]
    case.update(id=name + "-basket", payoff_list=[(K, cp) for cp in (1.0, -1.0) for K in (S0 / 2, S0, 3 * S0)])
    ref = lx.reference(case, case["payoff_list"])
    paths = [int(i) for i in np.flatnonzero(np.all([pj["usable"] for pj in ref["payoffs"]], axis=0))]
    assert len(paths) >= ref["n"] - 1
    strikes = np.array([K for K, _ in case["payoff_list"]])
    cps = np.array([cp for _, cp in case["payoff_list"]])
    seeds = {slot: [1.0 if q == k else 0.0 for q in range(NS - 1)] for k, slot in enumerate(SLOTS[:-1])}
    m = lc.model_of(case, S0, 1.0, seeds=seeds, n_partials=NS - 1)  # a strike seed is refused by the basket
    c = lc.config_of(case, paths, n_partials=NS - 1)
    res = (_ffi.hh_result * len(strikes))()
    term = np.zeros(len(paths) * ref["members"])
    hhlib.check(hhlib.lib.hh_mc_solve_basket(hhlib.handle, C.byref(m), C.byref(c), strikes.ctypes.data, cps.ctypes.data,
                                             len(strikes), res, term.ctypes.data))
    bad = []
    for j in range(len(strikes)):
        bad += etc.check_solve(worst, case, ref, j, paths, res[j], term if j == 0 else None, "device basket",
                               skip=("strike",))
    assert not bad, "\n".join(bad[:20])


# ---- (f) GENERATE ----------------------------------------------------------------------------------------------------

def generated(oracle, case, key, path_offset, n, name):
    """The reference on the normals the device draws for trajectories path_offset … + n − 1 of `key`'s stream.  The host
    cannot read the normals of kDomExactGbm, so they are restated at 50 digits from the Philox words by hh_rng.h's
    formulas (lc.exact_law_normals).  -> (case on the rounded normals — its reference gives usable, e64 and A —, the
    50-digit normals, the 50-digit run on them, dz[i] = PAIR_BAR·ε·|z_i|: what tests/test_gpu_rng_device.py allows
    normal_pair)"""
    z = lc.exact_law_normals(oracle, key, path_offset, n)
    with mp.workdps(lx.DPS):
        g = dict(case, id=f"{name}-generate-offset{path_offset}", z=[float(t) for t in z])
        want = lx.run(dict(g, z=z), mp.mpf, case["payoff_list"])
        dz = [PAIR_BAR * EPS * abs(float(t)) for t in z]
    return g, z, want, dz


def terminal_bars(case, ref, want, dz):
    """per member and path: the path bar plus what the normal's bar does to S_T — it enters x times |σ·√T|, and S = e^x"""
    sx = abs(case["sigma"]) * math.sqrt(case["T"])
    S = np.array([[float(w["S"][m][0]) for w in want] for m in range(ref["members"])])
    return etc.path_bar(ref["S_e64"], ref["S_A"]) + S * sx * np.array(dz)


@pytest.mark.parametrize("path_offset", [0, 1, 2**33 - 1])
@pytest.mark.parametrize("name", ["ref", "ref-compat-anti", "bench-anti"])
def test_generate(hhlib, oracle, worst, name, path_offset):
    """GENERATE, n_paths = 32, eight unit seeds.  An odd offset takes the second component of one Philox block and the
    first of the next (exact_pair_normals' odd branch); 2³³ − 1 carries into the counter's second word after the first
    trajectory.  The device's normal may miss its 50-digit restatement by PAIR_BAR·ε·|z| (tests/test_gpu_rng_device.py);
    that enters x multiplied by |σ·√T| and from there every output: the allowance of a path's number is the larger
    change of the 50-digit reference under z ± that bar, ADDED to the path bar; sums add their paths' allowances."""
    case = BY_ID[name]
    key, n = 0x1234567887654321 + path_offset % 7, 32
    g, z, want, dz = generated(oracle, case, key, path_offset, n, name)
    ref = lx.reference(g, case["payoff_list"])
    with mp.workdps(lx.DPS):
        moved = [lx.run(dict(g, z=[t + s * d for t, d in zip(z, dz)]), mp.mpf, case["payoff_list"]) for s in (1, -1)]
    bad = []
    for j, (strike, cp) in enumerate(case["payoff_list"]):
        paths = lc.usable_paths(ref, j)
        print(f"\n{g['id']} K={strike:g} cp={cp:+.0f}: {n - len(paths)} of {n} paths left out")
        assert n - len(paths) <= etc.MAX_UNUSABLE * n and len(paths) == n  # the solve draws all 32: none may be left out
        c = _ffi.make_config(GBM, EXACT, n, 1, antithetic=int(case["antithetic"]), seeds=[key], n_partials=NS,
                             path_offset=path_offset, compat_sqrt_alpha=int(case["compat_sqrt_alpha"]))
        res, term = solve(hhlib, lc.model_of(case, strike, cp), c)
        where = f"{g['id']} K={strike:g} cp={cp:+.0f}"
        sbar = terminal_bars(case, ref, want, dz)
        for m in range(ref["members"]):
            for i in range(n):
                bad.append(worst.check("GENERATE S_T", term[m * n + i], want[i]["S"][m][0], sbar[m][i], f"{where} path {i} member {m}"))
        pj = ref["payoffs"][j]
        with mp.workdps(lx.DPS):
            rows = [lx.ex._flat(w["payoffs"][j]["price"]) for w in want]
            allow = [[float(max(abs(a - b) for a in (lx.ex._flat(mv[i]["payoffs"][j]["price"])[s] for mv in moved)))
                      for s, b in enumerate(rows[i])] for i in range(n)]
            price, bar = etc.sum_of(rows, pj["price_e64"], pj["price_A"], paths, int(case["antithetic"]))
            price = [t / n for t in price]
        bar = (bar + np.sum([allow[i] for i in paths], axis=0)) / n
        bad.append(worst.check("GENERATE sum price", res.price, price[0], bar[0], where))
        for k in range(NS):
            bad.append(worst.check(f"GENERATE sum d/d{SLOTS[k]}", res.dprice[k], price[1 + k], bar[1 + k], where))
        bad += zero_columns(res, where)
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ---- whole ensembles in long double ----------------------------------------------------------------------------------

def need_long_double():
    if not np.finfo(LD).eps < 2.0**-60:
        pytest.skip("long double is no wider than double here")
    assert np.finfo(LD).eps < 2.0**-60


def ensemble(case, z, mirror):
    """-> (S_T in long double from the model's scalars, bar = 20·ε·S·max(1, A_x)),  A_x = |log S0| + (|r| + σ²/2)·m + |σ·√T·z|:
    the path bar's rule without e64"""
    S0, sig, r, T = (LD(case[k]) for k in ("S0", "sigma", "r_drift", "T"))
    s = np.sqrt(T)
    m = s if case["compat_sqrt_alpha"] else T
    mean = np.log(S0) + (r - sig * sig / 2) * m
    dev = (sig * s) * z.astype(LD)
    S = np.exp(mean - dev if mirror else mean + dev)
    A = float(abs(np.log(S0)) + (abs(r) + sig * sig / 2) * m) + np.abs(dev).astype(np.float64)
    return S, 20.0 * EPS * S.astype(np.float64) * np.maximum(1.0, A)


def check_ensemble(worst, kind, case, z, term, where):
    n = len(z)
    for member in range(2 if case["antithetic"] else 1):
        S, bar = ensemble(case, z, member == 1)
        ratio = np.abs(term[member * n:(member + 1) * n].astype(LD) - S).astype(np.float64) / bar
        i = int(np.argmax(ratio))
        note(worst, kind, ratio[i], f"{where} path {i} member {member}")
        assert ratio[i] <= 1.0, (where, i, member, term[member * n + i], S[i])


def check_sums(worst, kind, case, strike, cp, res, term, n, where):
    """sum_payoff against math.fsum of the payoffs of the device's OWN terminals, within the plain summation bound
    (n − 1)·ε·Σ|p| (a pair average is formed as the device forms it: the same two roundings); the price, discount·sum/n,
    against the same sum at that bound scaled and its own two roundings."""
    def payoffs(S):  # cp = ±1: cp·(S − K) is one rounding either way
        p = S - strike
        p *= cp
        return np.maximum(p, 0.0, out=p)

    p = payoffs(term[:n])
    if case["antithetic"]:
        p += payoffs(term[n:])
        p /= 2
    p = p[p != 0.0]
    exact = math.fsum(itertools.chain.from_iterable(part.tolist() for part in np.array_split(p, 64)))
    bar = (n - 1) * EPS * float(np.sum(p))
    assert bar > 0
    e = abs(res.sum_payoff - exact)
    note(worst, kind, e / bar, where)
    assert e <= bar, (where, res.sum_payoff, exact)
    want = case["discount"] * exact / n
    assert abs(res.price - want) <= case["discount"] * bar / n + 2 * EPS * abs(want), (where, res.price, want)


def check_at_50_digits(worst, kind, case, ref, want, extra, term, picks, n, where):
    """the picked trajectories (g = position in `ref`, i = index in the ensemble) against the 50-digit reference"""
    bars = etc.path_bar(ref["S_e64"], ref["S_A"]) + extra
    bad = []
    for member in range(ref["members"]):
        for g, i in enumerate(picks):
            bad.append(worst.check(kind, term[member * n + i], want[member][g], bars[member][g], f"{where} path {i} member {member}"))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


def picks_of(n, pairs, middle):
    """first and last lane (both trajectories of their first and last pair) of the first and the last full workgroup, one
    trajectory of every pair index jp of a middle one, and the whole ragged tail"""
    per = WG * pairs
    full = n // per
    out = []
    for wg in (0, full - 1):
        for jp in (0, pairs - 1):
            for tid in (0, 255):
                out += [(wg * pairs + jp) * WG + 2 * tid + j for j in (0, 1)]
    out += [(middle * pairs + jp) * WG + 2 * ((37 + 13 * jp) % 256) + (jp & 1) for jp in range(pairs)]
    out += list(range(full * per, n))
    assert len(set(out)) == len(out) and max(out) == n - 1
    return out


# ---- (g) ragged shapes of the 4-pair form ----------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("n", [511, 512, 513, 2047, 2048, 2049])
def test_ragged_shapes_of_the_four_pair_form(hhlib, worst, n, anti):
    """A workgroup of the 4-pair form takes 2048 trajectories, a pair index 512: one short of, at and one past both,
    REPLAY.  Every terminal against the long-double ensemble, the sums against fsum of the terminals' payoffs."""
    need_long_double()
    case = dict(BY_ID["bench-anti" if anti else "bench"])
    z = np.random.default_rng(n).standard_normal(n)
    c = _ffi.make_config(GBM, EXACT, n, 1, antithetic=anti, noise_mode=_ffi.HH_NOISE_REPLAY, replay=z)
    res, term = solve(hhlib, lc.model_of(case, 100.0, 1.0, seeds=None, n_partials=0), c)
    assert res.n_paths_done == n
    check_ensemble(worst, "ensemble S_T, 4 pairs", case, z, term, f"n={n} anti={anti}")
    check_sums(worst, "sum against fsum", case, 100.0, 1.0, res, term, n, f"n={n} anti={anti}")


# ---- (h) the 8-pair form ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def eight(hhlib):
    """one solve: 2048·512·8 + 700 trajectories, REPLAY, antithetic — 67 MB in, 134 MB out"""
    case = dict(BY_ID["bench-anti"])
    z = np.random.default_rng(8).standard_normal(N8)
    c = _ffi.make_config(GBM, EXACT, N8, 1, antithetic=1, noise_mode=_ffi.HH_NOISE_REPLAY, replay=z)
    res, term = solve(hhlib, lc.model_of(case, 100.0, 1.0, seeds=None, n_partials=0), c)
    assert res.n_paths_done == N8
    return case, z, res, term


def test_eight_pair_form_whole_ensemble(eight, worst):
    need_long_double()
    case, z, res, term = eight
    check_ensemble(worst, "ensemble S_T, 8 pairs", case, z, term, "8 pairs")


def test_eight_pair_form_at_50_digits_and_its_sums(eight, worst):
    """The first and last lane of the first and last full workgroup, one trajectory of each jp = 0…7 of workgroup 1024
    and the 700 of the ragged tail (workgroup 2048: pair 0 full, 188 of pair 1) at 50 digits; the sums against fsum."""
    case, z, res, term = eight
    picks = picks_of(N8, 8, 1024)
    g = dict(case, id="eight-pairs", z=[float(z[i]) for i in picks])
    ref = lx.reference(g, [(100.0, 1.0)])
    check_at_50_digits(worst, "S_T, 8 pairs", g, ref, ref["S"], 0.0, term, picks, N8, "8 pairs")
    check_sums(worst, "sum against fsum", case, 100.0, 1.0, res, term, N8, "8 pairs")


# ---- (i) the 64-pair form --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sixty_four(hhlib):
    """one solve with terminals: 2048·512·64 + 513 trajectories, GENERATE at path_offset 3 — 0.5 GB out"""
    case = dict(BY_ID["bench"])
    key = 0x0F1E2D3C4B5A6978
    c = _ffi.make_config(GBM, EXACT, N64, 1, seeds=[key], path_offset=3)
    res, term = solve(hhlib, lc.model_of(case, 120.0, 1.0, seeds=None, n_partials=0), c)
    assert res.n_paths_done == N64
    return case, key, res, term


def test_sixty_four_pair_form_at_50_digits_and_its_sums(sixty_four, oracle, worst):
    """One trajectory of each jp = 0…63 of workgroup 1024, the workgroup edges and the 513 of the ragged tail
    (workgroup 2048: pair 0 full, one trajectory of pair 1), each against the reference on its own normal as in
    test_generate (restated from the Philox words; the normal's bar enters S_T times |σ·√T|·S); the sums against fsum
    of the terminals' payoffs (strike 120: a fifth of 6.7·10⁷ terms are not zero)."""
    case, key, res, term = sixty_four
    picks = picks_of(N64, 64, 1024)
    with mp.workdps(lx.DPS):
        z = [lc.exact_law_normals(oracle, key, 3 + i, 1)[0] for i in picks]
        g = dict(case, id="sixty-four-pairs", z=[float(t) for t in z])
        want = lx.run(dict(g, z=z), mp.mpf, [(120.0, 1.0)])
        dz = [PAIR_BAR * EPS * abs(float(t)) for t in z]
    ref = lx.reference(g, [(120.0, 1.0)])
    extra = terminal_bars(case, ref, want, dz) - etc.path_bar(ref["S_e64"], ref["S_A"])
    check_at_50_digits(worst, "GENERATE S_T, 64 pairs", g, ref, [[w["S"][0][0] for w in want]], extra, term, picks, N64, "64 pairs")
    check_sums(worst, "sum against fsum", case, 120.0, 1.0, res, term, N64, "64 pairs")


# ---- (j) the LSM path grid -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anti", [0, 1])
@pytest.mark.parametrize("n_steps,T", [(1, 1 / 64), (2, 2 / 64), (7, 7 / 64), (30, 30 / 64), (100, 100 / 256)])
@pytest.mark.parametrize("tag", ["ref", "bench"])
def test_lsm_path_grid(hhlib, worst, tag, n_steps, T, anti):
    """gbm_grid_kernel through hh_lsm_solve's spot_grid (degree 1, 32 keys): every row of every path against the grid
    reference at its bar, row 0 == S0.  dt = T/n_steps is 1/64 or 1/256, so √dt is a power of two and the device's own
    normals are hh_wiener_fill(HH_LOGNORMAL, …)/√dt exactly (gbm_grid_kernel and wiener_fill_kernel<1> draw with the
    same key, counter and domain; the odd step counts take z1 of a pair whose z2 is unused).  The mirror is the device's
    exp(2a)·rcp(e) against the reference's recursion with −σ."""
    import torch
    case = dict(BY_ID[tag])
    n, dt = 32, T / n_steps
    sdt = math.sqrt(dt)
    assert dt in (1 / 64, 1 / 256) and sdt in (1 / 8, 1 / 16)
    buf = torch.zeros(hhlib.lib.hh_replay_elems(n, n_steps, GBM), dtype=torch.float64, device="cuda")
    hhlib.check(hhlib.lib.hh_wiener_fill(hhlib.handle, GBM, 0.0, T, n_steps, n, lc.GRID_SEEDS.ctypes.data, 0, buf.data_ptr()))
    hhlib.synchronize()
    z = np.ascontiguousarray(buf.cpu().numpy().reshape(n_steps, 256).T[:n] / sdt)
    assert np.all(np.abs(z) > 0) and np.all(np.abs(z) < 8.6)
    ref = lc.grid_reference(case, n_steps, T, z)
    m = _ffi.make_model(S0=case["S0"], sigma=case["sigma"], r=case["r_drift"], T=T, strike=case["S0"], cp=-1.0)
    c = _ffi.make_config(GBM, EXACT, n, n_steps, antithetic=anti, seeds=lc.GRID_SEEDS)
    ntot = n * (2 if anti else 1)
    tau, val, grid = np.zeros(ntot, dtype=np.int32), np.zeros(ntot), np.full((n_steps + 1, ntot), np.nan)
    res = _ffi.hh_lsm_result()
    hhlib.check(hhlib.lib.hh_lsm_solve(hhlib.handle, C.byref(m), C.byref(c), 1, math.exp(-case["r_drift"] * dt), C.byref(res),
                                       tau.ctypes.data, val.ctypes.data, grid.ctypes.data))
    assert res.n_paths_total == ntot
    bad = lc.check_grid(worst, "device", grid, ref, anti, f"{tag} steps={n_steps} anti={anti}")
    assert not bad, "\n".join(bad[:20])
