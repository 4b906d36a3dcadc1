"""Cases, residual and bar of the Broadie–Kaya exact-law tests (tests/golden/bk_law_exact.json, written by
tests/golden/make_bk_law_exact.py from oracle/bk_law_exact.py), shared by the host test (the fp64 oracle's samples) and
the device test (the kernels').

A sample x returned for the uniform u is held to the law it is drawn from:

    |F(x) − u|  <=  stop + E_alg + 20·max(e64, ε·A)

whatever way the root search went.  F is the exact conditional CDF of ∫V given (V0, V_T); around the stored quantile x*
it is u + Σ_{n=0…4} f⁽ⁿ⁾(x*)·Δⁿ⁺¹/(n+1)! with Δ = x − x*, and the remainder max|f⁽⁵⁾|·Δ⁶/720 (the fixture's bound holds for
all x) is ADDED to the residual; where that remainder is more than a hundredth of the bar F(x) is evaluated outright.
  stop    bk_atol where the search ended on |F_alg − u| <= atol (the secant's root was accepted), f(x*)·bk_atol where
          it ended by bracket width (bisection); nothing where it returned max_guess: that exit has no claim on u
  E_alg   |F_alg − F|: the sampler's truncated series with its own step against the law, both at 50 digits — AT THE
          SAMPLE: a search that stops on F_alg ends where |F − u| <= stop + E_alg, not at x*, and the series' error is
          a wave in x of length ~2π/(h·N), not a constant.  The fixture holds it (E_alg_reach) on equidistant points,
          no further apart than 0.2/(h·N), over the x with |F(x) − u| <= 2·(stop + E_alg(x*)) (`reach`: from 0 where u is no larger than that, as for
          u = 10⁻³ under the shipped controls); the bar takes the larger of the two points around the sample, and a
          sample outside `reach` fails whatever its residual.  (E_alg(x*) alone is not a bound a correct sampler
          meets: the fp64 oracle missed it by 12 % and 6 % at u = 10⁻³ of regime q2, where f is small and the sample
          0.01 from x*.)
  e64     what doubles cost that series at x* (moments, step, stopping rule and sum in numpy/scipy against 50 digits)
  ε·A     the recovery of ∫V from log S_T: with Z = 0, log S_T = log S0 + rT + (ρ/σ)(V_T − V0 − κθT) + (ρκ/σ − ½)·∫V;
          its terms carry an ulp each, A = f(x*)·(1 + Σ|terms|)/|ρκ/σ − ½| (the 1: the exp that makes S_T);
          0 for a sample that was never a spot
Nothing in the bar comes from the code under test."""
import json
import os

import mpmath as mp
import numpy as np

from oracle import bk_law_exact as bx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bk_law_exact.json")
EPS = 2.0 ** -53
DEC_BRANCH_SHIFT, DEC_BISECT, DEC_MAXGUESS = 8, 1, 2

with open(GOLDEN) as _f:
    DOC = json.load(_f)
CONTROLS = DOC["controls"]
REGIMES = DOC["regimes"]
CASES = DOC["cases"]
LAWS = {rec["id"]: rec for rec in DOC["laws"]}


def cases_of(regime):
    return [c for c in CASES if c["regime"] == regime]


def law_of(case):
    p = REGIMES[case["regime"]]
    return bx.Law(p["V0"], case["VT"], p["kappa"], p["theta"], p["sigma"], p["T"])


def integral_from_spot(case, S_T, S0=None):
    """∫V from the terminal spot of a trajectory with Z = 0, in mpmath"""
    p = REGIMES[case["regime"]]
    with mp.workdps(bx.DPS):
        k, th, sg, rho, r, T, V0 = (mp.mpf(p[n]) for n in ("kappa", "theta", "sigma", "rho", "r", "T", "V0"))
        S0 = mp.mpf(p["S0"] if S0 is None else S0)
        num = mp.log(mp.mpf(float(S_T))) - mp.log(S0) - r * T - rho / sg * (mp.mpf(case["VT"]) - V0 - k * th * T)
        return num / (rho * k / sg - mp.mpf(1) / 2)


def recovery_allowance(case, S0=None):
    """A of the bar: f(x*)·(1 + Σ|terms of log S_T|)/|ρκ/σ − ½|"""
    p = REGIMES[case["regime"]]
    x, f = float(mp.mpf(case["x"])), float(mp.mpf(case["f"]))
    coef = p["rho"] * p["kappa"] / p["sigma"] - 0.5
    assert abs(coef) >= 0.5
    S0 = p["S0"] if S0 is None else S0
    terms = abs(np.log(S0)) + abs(p["r"] * p["T"]) + 0.5 * x + abs(p["rho"] / p["sigma"]) * (
        case["VT"] + p["V0"] + p["kappa"] * p["theta"] * p["T"] + p["kappa"] * x)
    return f * (1.0 + terms) / abs(coef)


def e_alg_at(case, control, x):
    """the larger of E_alg at the two grid points of `reach` around x; None outside `reach`"""
    c = case["controls"][control]
    (lo, hi), grid = c["reach"], c["E_alg_reach"]
    if not lo <= x <= hi:
        return None
    i = min(int(float((mp.mpf(x) - lo) / (hi - lo)) * (len(grid) - 1)), len(grid) - 2)
    return max(grid[i], grid[i + 1])


def bar_of(case, control, decision, x, A=0.0):
    c, ctl = case["controls"][control], CONTROLS[control]
    branch = (int(decision) >> DEC_BRANCH_SHIFT) & 3
    stop = {0: ctl["bk_atol"], DEC_BISECT: float(mp.mpf(case["f"])) * ctl["bk_atol"]}.get(branch, 0.0)
    e_alg = e_alg_at(case, control, x)
    return stop + (c["E_alg"] if e_alg is None else e_alg) + 20.0 * max(c["e64"], EPS * A)


def residual_of(case, x, bar):
    """|F(x) − u| (and how it was formed) for a sample x given as an mpf"""
    with mp.workdps(bx.DPS):
        d = mp.mpf(x) - mp.mpf(case["x"])
        rem = mp.mpf(case["f5_bound"]) * d ** 6 / 720
        if rem <= bar / 100:
            taylor = mp.fsum(mp.mpf(case[k]) * d ** (n + 1) / mp.factorial(n + 1) for n, k in enumerate(("f", "f1", "f2", "f3", "f4")))
            return float(abs(taylor) + rem), "taylor"
        if not x > 0:
            return float(mp.mpf(case["u"])), "outright"
        law = law_of(case).build(max(mp.mpf(LAWS[case["law"]]["x_max"]), mp.mpf(x)))
        return float(abs(law.F(x) - mp.mpf(case["u"]))), "outright"


class Worst:
    """worst residual/bar per regime and control set, for the lines a module prints at its end"""

    def __init__(self, title):
        self.title, self.w = title, {}

    def check(self, case, control, x, decision, where, A=0.0):
        """-> None when the sample is inside its bar, a description when not"""
        bar = bar_of(case, control, decision, x, A)
        res, how = residual_of(case, x, bar)
        if e_alg_at(case, control, x) is None:
            res, how = max(res, 2 * bar), how + ", beyond the reach E_alg was taken over"
        key = (case["regime"], control)
        tag = f"{case['law']} u={case['u']:g} {where}"
        if res / bar > self.w.get(key, (-1.0, ""))[0]:
            self.w[key] = (res / bar, tag)
        if res <= bar:
            return None
        return (f"{control} {tag}: x = {mp.nstr(x, 17)}, x* = {case['x'][:19]}, |F(x) − u| = {res:.3g} ({how}), bar {bar:.3g}, "
                f"decision {int(decision):#x}")

    def report(self):
        for (regime, control), (ratio, where) in sorted(self.w.items()):
            print(f"\n{self.title} worst residual/bar, {regime} {control}: {ratio:.3g} ({where})")
