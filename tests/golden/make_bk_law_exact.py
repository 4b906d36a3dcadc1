"""Writes tests/golden/bk_law_exact.json: Broadie–Kaya samples' exact answers (oracle/bk_law_exact.py).
Run from the repository root: python tests/golden/make_bk_law_exact.py   (minutes, on up to 16 processes)

Cases: the nine regimes of tests/test_gpu_bk.py::PARAMS; V_T at the 0.001, 0.5 and 0.999 quantiles of its non-central
χ² law (scipy.stats.ncx2.ppf, kept to 12 significant digits); u from {10⁻³, 0.3, 0.5, 0.9, 0.999}: all five at the
median V_T, {10⁻³, 0.9} at the low one, {0.5, 0.999} at the high one — nine (V_T, u) pairs per regime; and the absorbed
variance: regime q2 (d = 0.13) at V_T = 2⁻¹⁰⁰⁰, the kernels' floor, u in {10⁻³, 0.5, 0.999}.  No case with a start
variance other than the model's V0: no entry point that takes the caller's (V_T, u, Z) takes one.

The far cases: regimes h252, intended and nu_one once more at their median V_T (laws `<regime>/q0.5/far`, listed behind
the regime's own three), with x_max from the Chernoff bound at 10⁻⁸ instead of 10⁻⁴ and u in {10⁻⁶, 1 − 10⁻⁶} (FAR_US).
Under the tight controls the low uniform sends every reading of the root search (bk_law_exact_cases.READINGS) to the
fall-back ladder, and 1 − 10⁻⁶ is the flat upper tail, where Order2's Steffensen slope is worst conditioned.  Under the
shipped controls these cases are nearly vacuous — E_alg there is hundreds of times u or 1 − u, so the bar admits nearly
any x in `reach` — and are kept for the record format alone.
The condition on a far case: in all eight readings and under both control sets the fp64 oracle's sample lies inside
`reach` and the search does not leave by the max_guess exit (held by tests/test_bk_law_exact_host.py); a case that fails
it has its u moved inward, 10⁻⁶ → 10⁻⁵ → 10⁻⁴.  Two did.  With u = 10⁻⁶ under the shipped controls, the midpoint
bisection of readings (0, 0, ·) returned 0.00874 for `intended` and 0.0326 for `nu_one`, beyond `reach` (which ends at
0.00810 and 0.0303: E_alg is a wave in x, and |F − u| there is 5.4e-4 and 1.0e-3, more than the twice
(stop + E_alg(x*)) that `reach` allows for).  At 10⁻⁵ all eight readings stay inside under both sets, and under the tight
set all eight still take the ladder.  h252 holds at 10⁻⁶, and every law holds at 1 − 10⁻⁶.
"""
import json
import math
import multiprocessing
import os
import sys

import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import bk_law_exact as bx  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "bk_law_exact.json")
CONTROLS = {
    "shipped": dict(bk_atol=1e-4, bk_cf_tol=1e-3, bk_n_sigma=5.0, bk_moment_h=1e-2, bk_newton_maxiter=10, bk_bisect_maxiter=100),
    # the caps as far as the decision word of hh_bk_decisions counts them: eight bits each
    "tight": dict(bk_atol=1e-10, bk_cf_tol=1e-10, bk_n_sigma=12.0, bk_moment_h=1e-2, bk_newton_maxiter=255, bk_bisect_maxiter=255),
}
US = {0.001: (1e-3, 0.9), 0.5: (1e-3, 0.3, 0.5, 0.9, 0.999), 0.999: (0.5, 0.999)}
ABSORBED_US = (1e-3, 0.5, 0.999)
FAR_REGIMES = ("h252", "intended", "nu_one")
FAR_US = {"h252": (1e-6, 1 - 1e-6), "intended": (1e-5, 1 - 1e-6), "nu_one": (1e-5, 1 - 1e-6)}   # (chosen as the docstring says)
FAR_TAIL = 8        # x_max of a far law: P(∫V > x_max) <= 10⁻⁸
DIGITS = 34
REACH_POINTS = 33   # at least; more where the series' error turns by more than REACH_PHASE between two of them
REACH_PHASE = 0.2


def regimes():
    from tests.test_gpu_bk import PARAMS
    return PARAMS


def variance_quantile(p, q):
    import scipy.stats as st
    k, th, sg, T, V0 = p["kappa"], p["theta"], p["sigma"], p["T"], p["V0"]
    em1 = -math.expm1(-k * T)
    d, lam = 4 * k * th / sg ** 2, 4 * k * math.exp(-k * T) * V0 / (sg ** 2 * em1)
    return float(f"{sg ** 2 * em1 / (4 * k) * st.ncx2.ppf(q, d, lam):.12g}")


def tasks():
    out = []
    for name, p in regimes().items():
        for q, us in US.items():
            out.append(dict(regime=name, law=f"{name}/q{q:g}", VT=variance_quantile(p, q), us=us))
        if name in FAR_REGIMES:
            out.append(dict(regime=name, law=f"{name}/q0.5/far", VT=variance_quantile(p, 0.5), us=FAR_US[name], tail=FAR_TAIL))
    out.append(dict(regime="q2", law="q2/absorbed", VT=bx.VT_FLOOR, us=ABSORBED_US))
    return out


def s(x):
    return mp.nstr(x, DIGITS)


def run(task):
    p = regimes()[task["regime"]]
    with mp.workdps(bx.DPS):
        law = bx.Law(p["V0"], task["VT"], p["kappa"], p["theta"], p["sigma"], p["T"])
        one, sym = law.phi(mp.mpf(0)), law.phi(mp.mpf(1)) - mp.conj(law.phi(mp.mpf(-1)))
        assert abs(one - 1) < mp.mpf(10) ** -35 and abs(sym) < mp.mpf(10) ** -35, (task, one, sym)
        mean, var = law.moments()
        # x_max: P(∫V > x_max) <= 10⁻⁴ (a far law: 10⁻⁸) by Chernoff, so the 0.999 (1 − 10⁻⁶) quantile lies below it
        tail = task.get("tail", 4)
        k, T, s2, *_ = law._consts()
        pole = (k * k + 4 * mp.pi ** 2 / (T * T)) / (2 * s2)
        x_max = min((mp.log(law.mgf(q * pole)) + mp.log(10 ** tail)) / (q * pole) for q in (0.3, 0.5, 0.7, 0.85, 0.95))
        law.build(x_max)
        assert law.F(x_max) > 1 - mp.mpf(10) ** -tail
        cases, xs = [], []
        for u in task["us"]:
            x = law.quantile(u, bx.start_of(law, u, 0.0, float(x_max)))
            resid = abs(law.F(x) - mp.mpf(u))
            assert 0 < x < x_max and resid < mp.mpf(10) ** -30, (task, u, x, resid)
            xs.append(x)
            cases.append(dict(law=task["law"], regime=task["regime"], VT=task["VT"], u=u, x=s(x), f=s(law.pdf(x)),
                              f1=s(law.pdf(x, 1)), f2=s(law.pdf(x, 2)), f3=s(law.pdf(x, 3)), f4=s(law.pdf(x, 4)), controls={}))
        halved = law.verify(xs + [x_max])
        assert halved < mp.mpf(10) ** -20, (task, halved)
        ladder = sorted([xs[0] / 4, xs[0] / 2] + xs + [(xs[-1] + x_max) / 2, x_max])
        b1, b5 = law.derivative_bound(1), law.derivative_bound(5)
        for name, ctl in CONTROLS.items():
            ser = bx.alg_series(law, ctl["bk_n_sigma"], ctl["bk_cf_tol"], ctl["bk_moment_h"])
            for c, x in zip(cases, xs):
                with mp.workdps(bx.DPS_ALG):
                    e_alg = abs(bx.alg_cdf(ser, x) - law.F(x))
                    f64, n64 = bx.alg_cdf_fp64(law.par, float(x), ctl["bk_n_sigma"], ctl["bk_cf_tol"], ctl["bk_moment_h"])
                    # (F_alg at the double nearest x*, which is where the doubles' sum was taken)
                    e64 = abs(mp.mpf(f64) - bx.alg_cdf(ser, mp.mpf(float(x))))
                    # E_alg where a sample can land: a search that stops on F_alg, not on F, ends where
                    # |F − u| <= stop + E_alg, and the series' error is a wave in x, not a constant.  Its values on
                    # equidistant points (the phase h·N·x of the last term 0.2 rad apart at most) over the x with |F(x) − u| <= w = 2·(stop + E_alg(x*)) — from 0 where
                    # u <= w, up to x_max where u + w >= F(x_max); the ends are doubles, by bisection.
                    w = float(2 * (max(1, law.pdf(x)) * mp.mpf(ctl["bk_atol"]) + e_alg))
                    lo = bx.start_of(law, c["u"] - w, 0.0, float(x)) if c["u"] > w else 0.0
                    hi = bx.start_of(law, c["u"] + w, float(x), float(x_max)) if c["u"] + w < float(law.F(x_max)) else float(x_max)
                    assert lo < x < hi, (task, c["u"], lo, hi)
                    n_grid = max(REACH_POINTS, int(mp.ceil((hi - lo) * ser["h"] * len(ser["re"]) / REACH_PHASE)) + 1)
                    assert n_grid <= 1025, (task, c["u"], n_grid)
                    grid = [mp.mpf(lo) + (mp.mpf(hi) - mp.mpf(lo)) * i / (n_grid - 1) for i in range(n_grid)]
                    e_grid = [float(abs(bx.alg_cdf(ser, t) - law.F(t))) for t in grid]
                    c["controls"][name] = dict(E_alg=float(e_alg), reach=[lo, hi], E_alg_reach=e_grid, e64=float(e64),
                                               terms=len(ser["re"]), terms_fp64=n64)
        for c in cases:
            c.update(f1_bound=float(b1), f5_bound=float(b5))
        rec = dict(id=task["law"], regime=task["regime"], VT=task["VT"], h=s(law.table["h"]), terms=len(law.table["re"]),
                   halved_step_difference=float(halved), mean=s(mean), variance=s(var), x_max=s(x_max),
                   ladder=[[s(x), s(law.F(x))] for x in ladder])
    return rec, cases


def main():
    todo = tasks()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1, len(todo))) as pool:
        done = pool.map(run, todo, chunksize=1)
    doc = dict(digits=DIGITS, controls=CONTROLS, regimes=regimes(), laws=[rec for rec, _ in done],
               cases=[c for _, cs in done for c in cs])
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(doc['laws'])} laws, {len(doc['cases'])} cases, {os.path.getsize(GOLDEN)} bytes")
    for name in CONTROLS:
        worst = max(doc["cases"], key=lambda c: c["controls"][name]["E_alg"])
        print(f"{name}: largest E_alg {worst['controls'][name]['E_alg']:.3g} ({worst['law']} u={worst['u']:g})")


if __name__ == "__main__":
    main()
