"""The golden Euler-tangent cases (tests/golden/euler_tangent_exact.json, written by tests/golden/
make_euler_tangent_exact.py) as the host and device tests read them, their 50-digit reference (oracle/euler_exact.py,
computed once per process and shared) and the bars both tests hold results to.

The bar of one path's number (S_T, payoff, price contribution, or one of their eight partials):

    bar = 20 · max(e64, ε·A),   ε = 2⁻⁵²

e64 is the distance of oracle/euler_exact.py's fp64 run from its 50-digit run on that path and slot, A the running
magnitude of that slot (the Σ|terms| of a first-order forward error bound, see that module).  Nothing in it comes from
the device or from the C oracle.  How large the bars are against the values they guard — 1e-14 … 5e-12 at the median,
below 1e-9 except where a partial has cancelled — is asserted by
tests/test_euler_tangent_exact_host.py::test_bars_are_fp64_sized.  The 20 is the project's factor for "a different but equally
careful fp64 sequence" (tests/carr_madan_cases.py): a reciprocal + Newton step in place of a division, the fused
per-step coefficients, fma contraction, another exp — each a few roundings per step, not an order of magnitude more.

A sum over n paths may miss by the bars of its terms plus (n − 1)·ε·Σ|terms| — the plain summation bound, whatever
the order of adding; the antithetic pair average counts as one more addition.  A direction assembled from seeds s_j on
the slots may miss by Σ_j |s_j|·bar_j.
"""
import json
import os

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "euler_tangent_exact.json")
SLOTS, NS, EPS = ex.SLOTS, ex.NS, ex.EPS
FACTOR = 20.0
MAX_UNUSABLE = 0.02       # of a case's paths
MIN_CLIP_FRACTION = 0.10  # of a clip case's path-steps: v <= 0


def expand(rec, noise, scale):
    """golden record -> case in the form oracle/euler_exact.py takes: dW[path][step][comp] = k / scale, exactly"""
    nz = noise[rec["noise"]]
    c = dict(rec["model"])
    c.update(id=rec["id"], tag=rec["tag"], dynamics=rec["dynamics"], n_steps=rec["n_steps"], em_split=rec["em_split"],
             antithetic=rec["antithetic"], clip=rec["clip"], flags_differ=rec["flags_differ"],
             payoff_list=[(p["strike"], p["cp"]) for p in rec["payoffs"]],
             digests=[p["price_sum"] for p in rec["payoffs"]])
    k = np.array(nz["k"], dtype=np.int64).reshape(nz["n_paths"], nz["n_steps"], nz["ncomp"])
    assert nz["n_steps"] == rec["n_steps"]
    c["dW"] = k.astype(np.float64) / float(scale)
    return c


def load_golden():
    doc = json.load(open(GOLDEN))
    assert tuple(doc["slots"]) == SLOTS
    return [expand(r, doc["noise"], doc["scale"]) for r in doc["cases"]]


CASES = load_golden() if os.path.exists(GOLDEN) else []
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]

_refs = {}


def reference(case):
    """the case's 50-digit reference and fp64 distances, computed once per process"""
    if case["id"] not in _refs:
        _refs[case["id"]] = ex.reference(case, case["payoff_list"])
    return _refs[case["id"]]


# ---- bars ----------------------------------------------------------------------------------------------------

def path_bar(e64, A):
    return FACTOR * np.maximum(e64, EPS * np.asarray(A))


def err(got, want):
    """|float − mpf| without rounding the exact value first"""
    return float(abs(mp.mpf(float(got)) - want))


def sum_of(rows, e64, A, paths, extra_adds=0):
    """Σ over `paths` of per-path rows [i][slot] (mpf) -> (sums [slot] mpf, bars [slot])"""
    n = len(paths)
    bars = path_bar(e64, A)
    sums, out = [], []
    with mp.workdps(ex.DPS):
        for s in range(len(rows[0])):
            sums.append(mp.fsum(rows[i][s] for i in paths))
            mag = float(mp.fsum(abs(rows[i][s]) for i in paths))
            out.append(sum(bars[i][s] for i in paths) + (n - 1 + extra_adds) * EPS * mag)
    return sums, np.array(out)


def assembled(seeds, values, bars):
    """direction with seeds[j] on slot j -> (Σ seeds_j·value_j, Σ |seeds_j|·bar_j); values/bars hold slot j at [1 + j]"""
    with mp.workdps(ex.DPS):
        want = mp.fsum(mp.mpf(float(s)) * values[1 + j] for j, s in enumerate(seeds))
    return want, float(sum(abs(float(s)) * bars[1 + j] for j, s in enumerate(seeds)))


def assert_bars_are_fp64_sized(ref, anti, limit, skip=()):
    """The bars of a reference against the VALUES they guard: what tests/test_euler_tangent_exact_host.py::
    test_bars_are_fp64_sized states, for any reference of euler_exact.reference's form.  `skip`: slots the caller
    holds against another scale."""
    ratios = []
    for pj in ref["payoffs"]:
        u = np.flatnonzero(pj["usable"])
        bars = path_bar(pj["price_e64"], pj["price_A"])[u]
        vals = np.array([[abs(float(t)) for t in row] for row in pj["price"]])[u]
        if not vals[:, 0].any():  # out of the money on every path: exact zeros, to be reproduced exactly
            assert not bars.any()
            continue
        sums, sbar = sum_of(pj["price"], pj["price_e64"], pj["price_A"], [int(i) for i in u], anti)
        for s, slot in enumerate(("price",) + SLOTS):
            if slot in skip:
                continue
            nz = vals[:, s] > 0
            scale = np.median(vals[nz, s]) if nz.any() else np.median(vals[vals[:, 0] > 0, 0])
            assert np.all(bars[:, s] <= limit * np.maximum(vals[:, s], scale)), slot
            ratios.append(bars[nz, s] / vals[nz, s])
            mag = vals[:, s].sum()
            assert sbar[s] <= limit * max(mag, scale), slot
            if abs(float(sums[s])) >= mag / 10:
                assert sbar[s] <= limit * max(abs(float(sums[s])), scale), slot
    ratios = np.concatenate(ratios)
    assert np.median(ratios) <= 1e-11
    assert np.mean(ratios <= 1e-9) >= 0.95
    sbar = path_bar(ref["S_e64"], ref["S_A"])
    S = np.array([[float(t) for t in row] for row in ref["S"]])
    assert np.all(sbar <= 1e-10 * S)


class Worst:
    """worst error/bar per kind of comparison, for the line a module prints at its end"""

    def __init__(self, title):
        self.title, self.w = title, {}

    def check(self, kind, got, want, bar, where):
        """note the comparison; -> None when inside the bar, a description when not"""
        e = err(got, want)
        ratio = e / bar if bar > 0 else (0.0 if e == 0 else float("inf"))
        if ratio > self.w.get(kind, (-1.0, ""))[0]:
            self.w[kind] = (ratio, where)
        return None if e <= bar else f"{kind} {where}: got {float(got)!r}, want {mp.nstr(want, 20)}, error/bar {ratio:.3g}"

    def report(self):
        for k, (ratio, where) in sorted(self.w.items()):
            print(f"\n{self.title} worst error/bar, {k}: {ratio:.3g} ({where})")


# ---- the C structs of a case -----------------------------------------------------------------------------------

GBM, HES = _ffi.HH_LOGNORMAL, _ffi.HH_HESTON
UNIT = {name: [1.0 if j == k else 0.0 for j in range(NS)] for k, name in enumerate(SLOTS)}


def dyn_of(case):
    return HES if case["dynamics"] == "heston" else GBM


def model_of(case, strike, cp, seeds=UNIT, n_partials=NS):
    return _ffi.make_model(S0=case["S0"], V0=case["V0"], kappa=case["kappa"], theta=case["theta"], sigma=case["sigma"],
                           rho=case["rho"], r=case["r_drift"], T=case["T"], strike=strike, cp=cp,
                           discount=case["discount"], seeds=seeds, n_partials=n_partials)


def replay_of(case, paths, path_major):
    """the increments of `paths` as a REPLAY buffer: dW[path][step][comp], or tile-major [tile][step][comp][256]"""
    dW = np.ascontiguousarray(case["dW"][list(paths)])
    if path_major:
        return dW
    n, steps, nc = dW.shape
    tiles = (n + 255) // 256
    out = np.zeros((tiles * 256, steps, nc))
    out[:n] = dW
    return np.ascontiguousarray(out.reshape(tiles, 256, steps, nc).transpose(0, 2, 3, 1))


def config_of(case, paths, path_major=False, n_partials=NS):
    return _ffi.make_config(dyn_of(case), _ffi.HH_EULER_MARUYAMA, len(paths), case["n_steps"],
                            antithetic=int(case["antithetic"]), em_split=int(case["em_split"]),
                            noise_mode=_ffi.HH_NOISE_REPLAY, replay=replay_of(case, paths, path_major),
                            replay_layout=_ffi.HH_REPLAY_PATH_MAJOR if path_major else _ffi.HH_REPLAY_TILE_MAJOR,
                            n_partials=n_partials)


def check_solve(worst, case, ref, j, paths, res, term, who, skip=()):
    """One solve over `paths` (all usable) of payoff j against the reference: every terminal to its per-path bar; the
    undiscounted sum, the price and the eight unit-seed partials to the sum bar (a single path: its own bar).
    -> list of misses"""
    pj, n, bad = ref["payoffs"][j], len(paths), []
    where = f"{case['id']} K={pj['strike']:g} cp={pj['cp']:+.0f} {who} paths={paths[0]}..{paths[-1]}"
    if term is not None:
        sbar = path_bar(ref["S_e64"], ref["S_A"])
        for m in range(ref["members"]):
            for q, i in enumerate(paths):
                bad.append(worst.check("S_T", term[m * n + q], ref["S"][m][i], sbar[m][i], f"{where} path {i} member {m}"))
    anti = int(case["antithetic"])
    pay, pbar = sum_of(pj["payoff"], pj["payoff_e64"], pj["payoff_A"], paths, anti)
    kind = "path" if n == 1 else "sum"
    bad.append(worst.check(f"{kind} payoff", res.sum_payoff, pay[0], pbar[0], where))
    price, bar = sum_of(pj["price"], pj["price_e64"], pj["price_A"], paths, anti)
    with mp.workdps(ex.DPS):
        price = [t / n for t in price]  # discount · mean(payoffs), montecarlo.jl:490
    bad.append(worst.check(f"{kind} price", res.price, price[0], bar[0] / n, where))
    for k in range(NS):
        if SLOTS[k] in skip:
            continue
        bad.append(worst.check(f"{kind} d/d{SLOTS[k]}", res.dprice[k], price[1 + k], bar[1 + k] / n, where))
    return [b for b in bad if b]
