"""The golden lognormal cases (tests/golden/lognormal_exact.json, written by tests/golden/make_lognormal_exact.py) as
the host and device tests read them, and their 50-digit reference (oracle/lognormal_exact.py, computed once per process
and shared).  The bars are tests/euler_tangent_cases.py's — path_bar = 20·max(e64, ε·A), sum_of, assembled — imported,
not restated; so are the usable-path rule, MAX_UNUSABLE and the Worst report.

A case is a model (S0, σ, r, T, discount), the flag compat_sqrt_alpha, the antithetic flag and a list of payoffs; every
case reads the same 32 standard normals, stored as integers k with z = k·2⁻⁴⁰ (exact in a double on every machine): 26
draws of numpy's generator, 0.0, −0.0 (an index list: an integer has no signed zero), ±8.5 — beyond the 8.57 that
normal_pair can reach only at u1 = 2⁻⁵³ — and 513·2⁻⁴⁰, −2⁻⁴⁰, both below 2⁻³⁰.

The grid cases take a golden model's scalars and the normals of 32 Philox keys (GRID_SEEDS): the C oracle and the device
draw them themselves, so the tests read them back (oracle.normal_pair; hh_wiener_fill divided by a power-of-two √dt)
and evaluate the reference on those doubles.
"""
import json
import os

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import lognormal_exact as lx
from tests import euler_tangent_cases as etc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lognormal_exact.json")
SLOTS, NS, EPS = lx.SLOTS, lx.NS, etc.EPS
GBM, EXACT = _ffi.HH_LOGNORMAL, _ffi.HH_EXACT_LAW
ZERO_SLOTS = ("V0", "kappa", "theta")  # nothing of the lognormal law reads them: exact zeros
GRID_SEEDS = np.arange(1, 33, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(7)


def normals_of(doc):
    z = np.array(doc["normals"]["k"], dtype=np.int64).astype(np.float64) / float(doc["scale"])
    for i in doc["normals"]["neg_zero"]:
        assert z[i] == 0.0
        z[i] = -0.0
    return z


def expand(rec, z):
    c = dict(rec["model"])
    c.update(V0=0.0, kappa=0.0, theta=0.0, rho=0.0, id=rec["id"], tag=rec["tag"],
             compat_sqrt_alpha=rec["compat_sqrt_alpha"], antithetic=rec["antithetic"], z=[float(t) for t in z],
             payoff_list=[(p["strike"], p["cp"]) for p in rec["payoffs"]],
             digests=[p.get("price_sum") for p in rec["payoffs"]])
    return c


def load_golden():
    doc = json.load(open(GOLDEN))
    assert tuple(doc["slots"]) == SLOTS
    z = normals_of(doc)
    return [expand(r, z) for r in doc["cases"]]


CASES = load_golden() if os.path.exists(GOLDEN) else []
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]

_refs, _grids = {}, {}


def reference(case):
    """the case's 50-digit reference and fp64 distances, computed once per process"""
    if case["id"] not in _refs:
        _refs[case["id"]] = lx.reference(case, case["payoff_list"])
    return _refs[case["id"]]


def grid_reference(case, n_steps, T, z):
    """the grid reference of a case's model on z[path][step], both members (the first member is the plain run), once per
    process and (model, n_steps, T)"""
    key = (case["tag"], n_steps, T, z.tobytes())
    if key not in _grids:
        g = dict(case, n_steps=n_steps, T=T, antithetic=1, z=[[float(t) for t in row] for row in z])
        _grids[key] = lx.grid_reference(g)
    return _grids[key]


def usable_paths(ref, j):
    return [int(i) for i in np.flatnonzero(ref["payoffs"][j]["usable"])]


def model_of(case, strike, cp, seeds=etc.UNIT, n_partials=NS):
    return etc.model_of(case, strike, cp, seeds=seeds, n_partials=n_partials)


def config_of(case, paths, n_partials=NS):
    """REPLAY of the normals of `paths`: one double per trajectory"""
    z = np.array([case["z"][i] for i in paths])
    return _ffi.make_config(GBM, EXACT, len(paths), 1, antithetic=int(case["antithetic"]),
                            noise_mode=_ffi.HH_NOISE_REPLAY, replay=z, n_partials=n_partials,
                            compat_sqrt_alpha=int(case["compat_sqrt_alpha"]))


def check_grid(worst, who, got, ref, anti, where):
    """got[(k), member·n + path] against the grid reference, every row of every path; row 0 is S0 itself"""
    n = len(ref["W"][0])
    bars = etc.path_bar(ref["e64"], ref["A"])
    bad = []
    for m in range(2 if anti else 1):
        for i in range(n):
            if got[0][m * n + i] != float(ref["W"][m][i][0]):
                bad.append(f"{who} {where}: row 0 of path {i} member {m} is {got[0][m * n + i]!r}")
            for k in range(1, got.shape[0]):
                bad.append(worst.check(f"grid {'mirror' if m else 'path'}", got[k][m * n + i], ref["W"][m][i][k],
                                       bars[m][i][k], f"{who} {where} path {i} row {k}"))
    return [b for b in bad if b]


# ---- the device's normals at 50 digits -------------------------------------------------------------------------------

def box_muller(words):
    """hh_rng.h's normal_pair on one Philox block, by its formulas at the working precision: u1 = (w01 >> 12 + 1/2)·2⁻⁵²,
    the angle π·t with t = 2·u2, r = √(−2 ln u1); z1 = r·cos, z2 = r·sin"""
    w = [int(t) for t in words]
    u1 = (mp.mpf(((w[1] << 32) | w[0]) >> 12) + mp.mpf(0.5)) * mp.mpf(2) ** -52
    t = 2 * (mp.mpf(((w[3] << 32) | w[2]) >> 12) + mp.mpf(0.5)) * mp.mpf(2) ** -52
    r = mp.sqrt(-2 * mp.log(u1))
    return r * mp.cospi(t), r * mp.sinpi(t)


def exact_law_normals(oracle, key, path_offset, n):
    """the normals of trajectories path_offset … path_offset + n − 1 of the exact law's ONE stream (hh_sim.h,
    exact_pair_normals): trajectory G takes component G & 1 of the block with counter (G >> 1, G >> 33, 0, 1)"""
    out, blocks = [], {}
    with mp.workdps(lx.DPS):
        for G in range(path_offset, path_offset + n):
            ctr = ((G >> 1) & 0xFFFFFFFF, G >> 33, 0, 1)
            if ctr not in blocks:
                blocks[ctr] = box_muller(oracle.philox(ctr, (key & 0xFFFFFFFF, key >> 32)))
            out.append(blocks[ctr][G & 1])
    return out
