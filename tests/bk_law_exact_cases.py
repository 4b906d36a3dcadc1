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
Nothing in the bar comes from the code under test.

THE EIGHT READINGS of the reference's two `find_zero` calls (READINGS: hh_config.bk_root_form, bk_bracket_form, bk_caps;
oracle/bk_oracle.py has the table) are held to the same bar.  E_alg, e64 and `reach` describe the series, which no
reading touches; only `stop` belongs to the search, and it is read off the decision word's branch alike in all eight:
  branch 0  the first search was accepted: bk_atol, in every reading.  The secant accepts on |f| <= atol.  Order2 also
            accepts on |f| <= max(atol, 4ε|x|), and, when its iterates stall, on |f| <= ∛tol — but an accepted iterate
            stands only if it passes the reference's own test once more: `if (ok && !(xb < 0.0 || fabs(fb) > p.atol))
            break;` in tail_whole_trajectory (csrc/hh_bk.hip), `if ok and not (sol < 0 or abs(fsol) > atol)` in
            bk_oracle.inverse_cdf.  (4ε|x| is far below either atol of CONTROLS.)
  branch 1  the fall-back ladder, either bisection: f(x*)·bk_atol.  The midpoint form ends on `xb - xa <= p.atol`
            (`stop = f == 0.0 || xb - xa <= p.atol || …`) and returns the middle.  The bit-pattern form ends at adjacent
            floats (`!(xa < mid && mid < xb)`) and returns the end with the smaller residual, so its bracket is narrower
            than atol by ten orders — and it still gets no tighter term.  One ulp, f(x*)·|x|·2⁻⁵², was tried: the fp64
            oracle misses it by 6 % (short_T/q0.5, u = 0.999, tight, reading (1, 1, 1): 3.69e-11 against 3.47e-11),
            because the sign of a residual at adjacent floats is decided by fp64 noise in the series, a little above
            the 20·e64 taken at x*.  (No cap of CONTROLS ends a bisection early: the midpoint form needs a few dozen
            halvings, the bit-pattern form ~62, against caps of 100 and 255.)
  branch 2  max_guess was returned: nothing.
The far cases (laws `<regime>/q0.5/far`: u = 10⁻⁶ — 10⁻⁵ in two — and 1 − 10⁻⁶) ride with their regime's cases."""
import json
import os

import mpmath as mp
import numpy as np

from oracle import bk_law_exact as bx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bk_law_exact.json")
EPS = 2.0 ** -53
DEC_BRANCH_SHIFT, DEC_BISECT, DEC_MAXGUESS = 8, 1, 2
DEC_ITERS_SHIFT = 16
READINGS = [(rf, bf, cp) for rf in (0, 1) for bf in (0, 1) for cp in (0, 1)]  # (bk_root_form, bk_bracket_form, bk_caps)

with open(GOLDEN) as _f:
    DOC = json.load(_f)
CONTROLS = DOC["controls"]
REGIMES = DOC["regimes"]
CASES = DOC["cases"]
LAWS = {rec["id"]: rec for rec in DOC["laws"]}


def cases_of(regime):
    return [c for c in CASES if c["regime"] == regime]


def is_far(case):
    return case["law"].endswith("/far")


FAR_LOW = [c for c in CASES if is_far(c) and c["u"] < 0.5]   # u = 10⁻⁶ (10⁻⁵ where the maker moved it): the ladder, tight set


def branch_of(decision):
    return (int(decision) >> DEC_BRANCH_SHIFT) & 3


def iterations_of(decision):
    return (int(decision) >> DEC_ITERS_SHIFT) & 0xff


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


_BUILT, _RESIDUALS = {}, {}


def _built_law(case, x):
    """the case's law with its table built up to x_max (kept: seconds each), or further for an x beyond it"""
    x_max = mp.mpf(LAWS[case["law"]]["x_max"])
    if x > x_max:
        return law_of(case).build(mp.mpf(x))
    if case["law"] not in _BUILT:
        _BUILT[case["law"]] = law_of(case).build(x_max)
    return _BUILT[case["law"]]


def residual_of(case, x, bar):
    """|F(x) − u| (and how it was formed) for a sample x given as an mpf.  Kept per (case, x, how): readings of the
    root search that walk the same path return the same bits."""
    with mp.workdps(bx.DPS):
        x = mp.mpf(x)
        d = x - mp.mpf(case["x"])
        rem = mp.mpf(case["f5_bound"]) * d ** 6 / 720
        how = "taylor" if rem <= bar / 100 else "outright"
        key = (case["law"], case["u"], x, how)
        if key not in _RESIDUALS:
            if how == "taylor":
                taylor = mp.fsum(mp.mpf(case[k]) * d ** (n + 1) / mp.factorial(n + 1) for n, k in enumerate(("f", "f1", "f2", "f3", "f4")))
                _RESIDUALS[key] = float(abs(taylor) + rem)
            elif not x > 0:
                _RESIDUALS[key] = float(mp.mpf(case["u"]))
            else:
                _RESIDUALS[key] = float(abs(_built_law(case, x).F(x) - mp.mpf(case["u"])))
        return _RESIDUALS[key], how


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
