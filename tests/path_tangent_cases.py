"""Pathwise derivatives of the path payoffs (include/hedgehog_mc.h, "Pathwise derivatives of path-dependent payoffs"): what
the host and the device tests share.

`run` is a restatement for oracle.euler_exact.reference(case, payoffs, run=run): the Euler scheme of that module, built
from its Dual rules one primitive at a time (never from the device's fused per-step map), which keeps on every monitoring
date the five statistics of enum hh_path_stat AS DUALS over the eight SLOTS — so the tangent of a statistic along every
slot, the passive ones (S0, r_drift) included, falls out of the sum, product and exp rules alone — and the date rows
K_MAX, K_MIN, SUM_KS.  The payoff rules are those rules again: max(·, 0) through dmax0, the geometric mean through dexp.

Comparisons.  Beside v > 0, K_v > 0 and itm, every "new extreme?" comparison S_j > MAX (S_j < MIN) is recorded with the
difference, its magnitude and whether it was taken, so euler_exact._usable leaves out a path on which fp64 and 50 digits
could pick different dates.  The tie rule is the header's: replaced only when STRICTLY greater (less).

Bars: tests/euler_tangent_cases.py's — path_bar per number, sum_of for sums, assembled for directions.  Nothing here
widens them.

One walk serves the four (include_start, antithetic) variants of a (model, shape): the states on the dates do not depend
on either, the mirror is the second member.  The walks are cached per process.
"""
import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex
from tests import euler_tangent_cases as tc
from tests import path_bridge_cases as bc

SLOTS, NS = ex.SLOTS, ex.NS
VANILLA, ARITH, GEOM = _ffi.HH_PAYOFF_VANILLA, _ffi.HH_PAYOFF_ASIAN_ARITH, _ffi.HH_PAYOFF_ASIAN_GEOM
LB_FLOAT, LB_FIXED = _ffi.HH_PAYOFF_LOOKBACK_FLOAT, _ffi.HH_PAYOFF_LOOKBACK_FIXED
STATS = ("SUM_S", "SUM_X", "MAX_S", "MIN_S", "S_T")  # enum hh_path_stat, and enum hh_path_tangent_row in this order
BASIS_SLOT = {_ffi.HH_BASIS_V0: SLOTS.index("V0"), _ffi.HH_BASIS_KAPPA: SLOTS.index("kappa"),
              _ffi.HH_BASIS_THETA: SLOTS.index("theta"), _ffi.HH_BASIS_SIGMA: SLOTS.index("sigma")}
MAX_UNUSABLE = tc.MAX_UNUSABLE
MIN_CLIP_FRACTION = bc.MIN_CLIP_FRACTION
N_PATHS = 65  # a full wave plus one lane
SHAPES = ((1, 1), (5, 1), (6, 3))  # (n_steps, monitor_every); 5 half-reads the Philox block of two lognormal steps

H = dict(bc.H252, discount=0.97)
# (the offsets of the two classic cases: of 0 .. 11 the ones with the smallest bars against the values they guard —
# euler_tangent_cases.assert_bars_are_fp64_sized's ratio, 1.1e-10 and 8.4e-11 — where offset 0 has a path with a bar of
# 3.4e-9 and 2.5e-9 of the value it guards: a condition on the inputs, found with the reference alone)
MODELS = {  # name -> (model, dynamics, em_split, seed offset)
    "lognormal": (dict(H, sigma=0.2), "lognormal", 1, 0),
    "heston-split": (H, "heston", 1, 0),
    "heston-classic": (H, "heston", 0, 4),
    "heston-classic-clipped": (dict(bc.CLIPPED, discount=0.97), "heston", 0, 7),
}
# (kind, strike, cp): each kind with a strike has paths on both sides of it (asserted by the host test)
PAYOFFS = ((VANILLA, 100.0, 1.0), (VANILLA, 101.0, -1.0), (ARITH, 100.0, 1.0), (ARITH, 101.0, -1.0), (GEOM, 100.0, 1.0),
           (GEOM, 99.0, -1.0), (LB_FLOAT, 0.0, 1.0), (LB_FLOAT, 0.0, -1.0), (LB_FIXED, 106.0, 1.0), (LB_FIXED, 95.0, -1.0))


def seeds_of(name):
    """65 seeds per model; the offset is one for which the reference keeps all but at most one path of every case (the host
    test asserts it on the oracle's increments)"""
    return np.arange(1, N_PATHS + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(MODELS[name][3])


def case_of(name, shape, start, anti, dW, payoffs=PAYOFFS):
    model, dyn, split, _ = MODELS[name]
    steps, every = shape
    return dict(model, id=f"{name}-{steps}x{every}-start{start}-anti{anti}",
                walk_key=(name, shape, hash(np.ascontiguousarray(dW).tobytes())), dynamics=dyn, em_split=split, n_steps=steps, monitor_every=every, include_start=start, antithetic=anti, dW=dW,
                kinds=[k for k, _, _ in payoffs], payoff_list=[(K, cp) for _, K, cp in payoffs], rows={})


# ---- the restatement -------------------------------------------------------------------------------------------------

def _step(case, p, x, v, d, record):
    """one step of euler_exact.heston_path / gbm_path, in its words"""
    dt = p["dt"]
    if case["dynamics"] == "heston":
        vp = ex.dmax0(v, record, "v")
        Kx = x + (p["r_drift"] - vp * p["half"]) * dt
        Kv = v + (p["kappa"] * (p["theta"] - vp)) * dt
        sq = ex.dsqrt_clipped(ex.dmax0(Kv, record, "Kv") if case["em_split"] else vp)
        return Kx + sq * d[0], Kv + (p["sigma"] * sq) * d[1]
    drift = p["r_drift"] - (p["sigma"] * p["sigma"]) * p["half"]
    return (x + drift * dt) + p["sigma"] * d[0], v


_walks = {}


def _dates(case, num):
    """per path and member: the comparison record of the steps and the Duals x on the dates every, 2·every, …, n_steps, and
    x0; both members always, cached"""
    key = (case["walk_key"], num is float)
    if key not in _walks:
        p = ex._model(case, num)
        out = []
        for rows in case["dW"]:
            dW = [[num(float(t)) for t in row] for row in rows]
            members = []
            for sign in (1, -1):
                rec, xs = [], []
                x, v = ex.dlog(p["S0"]), p["V0"]
                x0 = x
                for k, row in enumerate(dW):
                    x, v = _step(case, p, x, v, [sign * t for t in row], rec)
                    if (k + 1) % case["monitor_every"] == 0:
                        xs.append((k + 1, x))
                members.append((rec, x0, xs))
            out.append(members)
        _walks[key] = (p, out)
    return _walks[key]


def _statistics(x0, xs, start, record, num):
    """Monitor's rules on the dates: the first term starts a sum, every later date takes one addition; an extreme is
    replaced when the date's S is strictly greater (less).  -> dict of Duals, and K_MAX, K_MIN (ints), SUM_KS (Dual)"""
    dates = ([(0, x0)] if start else []) + list(xs)
    st = None
    for k, x in dates:
        S = ex.dexp(x)
        if st is None:
            st = dict(SUM_S=S, SUM_X=x, MAX_S=S, MIN_S=S, S_T=S, K_MAX=k, K_MIN=k, SUM_KS=S * num(k))
            continue
        up, dn = S - st["MAX_S"], st["MIN_S"] - S
        record.append(("max", up.v, up.a, up.v > 0))
        record.append(("min", dn.v, dn.a, dn.v > 0))
        if up.v > 0:
            st["MAX_S"], st["K_MAX"] = S, k
        if dn.v > 0:
            st["MIN_S"], st["K_MIN"] = S, k
        st["SUM_S"], st["SUM_X"], st["S_T"] = st["SUM_S"] + S, st["SUM_X"] + x, S
        st["SUM_KS"] = st["SUM_KS"] + S * num(k)
    return st


def _payoff(kind, st, K, cp, n_mon, record, num):
    """the header's table on the statistics, each line by the Dual rules"""
    inv_n = num(1) / n_mon
    if kind == LB_FLOAT:
        return st["S_T"] - st["MIN_S"] if cp > 0 else st["MAX_S"] - st["S_T"]
    if kind == LB_FIXED:
        return ex.dmax0(st["MAX_S"] - K if cp > 0 else K - st["MIN_S"], record, "itm")
    base = {VANILLA: lambda: st["S_T"], ARITH: lambda: st["SUM_S"] * inv_n, GEOM: lambda: ex.dexp(st["SUM_X"] * inv_n)}[kind]()
    return ex.dmax0((base - K) * cp, record, "itm")


def run(case, num, payoffs):
    """euler_exact.run's output for the path payoffs case["kinds"][j] at (strike, cp) = payoffs[j]; the statistics of every
    member go to case["rows"]["mp" | "f64"][path][member]."""
    p, walks = _dates(case, num)
    members = 2 if case["antithetic"] else 1
    start = case["include_start"]
    n_mon = case["n_steps"] // case["monitor_every"] + (1 if start else 0)
    out, stash = [], []
    for walk in walks:
        sim_rec, ext_rec, sts = [], [], []
        for rec, x0, xs in walk[:members]:
            sim_rec += rec
            sts.append(_statistics(x0, xs, start, ext_rec, num))
        res = dict(sim_record=sim_rec + ext_rec, S=[(st["S_T"].v, st["S_T"].a) for st in sts], payoffs=[])
        for kind, (strike, cp) in zip(case["kinds"], payoffs):
            K = ex.Dual.input(num(strike), NS - 1)
            rec = []
            pays = [_payoff(kind, st, K, num(cp), n_mon, rec, num) for st in sts]
            pay = pays[0] if members == 1 else (pays[0] + pays[1]) * num(0.5)
            res["payoffs"].append(dict(payoff=pay, price=p["discount"] * pay, record=rec))
        out.append(res)
        stash.append(sts)
    case["rows"]["f64" if num is float else "mp"] = stash
    return out


_refs = {}


def reference(case):
    """euler_exact.reference of the case under `run`, once per process, and of the statistics of every member:
      usable_sim[i]        the path's step and extreme comparisons are decided (no payoff's itm in it)
      usable_all[i]        … and every payoff's
      k_max, k_min         int arrays [member][path]
      stat[name]           want [member][path][1 + NS] mpf (value, then the partials in SLOTS order), e64, A float arrays;
                           name in STATS + ("SUM_KS",)"""
    key = (case["id"], case["walk_key"])
    if key in _refs:
        return _refs[key]
    ref = ex.reference(case, case["payoff_list"], run=run)
    rm, r6 = case["rows"]["mp"], case["rows"]["f64"]
    members, n = ref["members"], ref["n"]
    with mp.workdps(ex.DPS):
        ref["k_max"] = np.array([[rm[i][m]["K_MAX"] for i in range(n)] for m in range(members)])
        ref["k_min"] = np.array([[rm[i][m]["K_MIN"] for i in range(n)] for m in range(members)])
        ref["stat"] = {}
        for name in STATS + ("SUM_KS",):
            want = [[ex._flat(rm[i][m][name]) for i in range(n)] for m in range(members)]
            A = np.array([[[float(rm[i][m][name].a)] + [float(t) for t in rm[i][m][name].ad] for i in range(n)]
                          for m in range(members)])
            e64 = np.array([[[ex._e64(g, w) for g, w in zip(ex._flat(r6[i][m][name]), want[m][i])] for i in range(n)]
                            for m in range(members)])
            ref["stat"][name] = dict(want=want, A=A, e64=e64)
    # a path whose payoffs are all out of the money still has decided step and extreme comparisons: any payoff without
    # an itm comparison (the floating lookback) carries exactly them
    j_float = case["kinds"].index(LB_FLOAT)
    ref["usable_sim"] = ref["payoffs"][j_float]["usable"]
    ref["usable_all"] = np.logical_and.reduce([pj["usable"] for pj in ref["payoffs"]])
    _refs[key] = ref
    return ref


def increments(oracle, name, steps):
    """the increments of the model's 65 seeds from the oracle's host fill: dW[path][step][comp]"""
    model, dyn, _, _ = MODELS[name]
    heston = dyn == "heston"
    tiled = oracle.wiener_fill(_ffi.HH_HESTON if heston else _ffi.HH_LOGNORMAL, model["rho"], model["T"], steps, seeds_of(name))
    return bc.increments_of(tiled, N_PATHS, steps, 2 if heston else 1)


def n_mon_of(case):
    return case["n_steps"] // case["monitor_every"] + (1 if case["include_start"] else 0)
