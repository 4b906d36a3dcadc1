"""The Euler–Maruyama scheme of the reference with its forward-mode tangent, one primitive at a time, generic in the
number type: `mpmath.mpf` at 50 digits is the reference the tests hold the device and oracle/hh_oracle.c to, Python
`float` is "the same formulas in fp64" whose distance from the 50-digit run sizes the bars (as oracle/carr_madan_fp64.py
does for Carr–Madan).  TEST INFRASTRUCTURE ONLY.

Written from the reference's formulas:
  LogHestonProblem / LogGBMProblem   src/distributions/heston.jl:7-52
  EM step  K = u + dt·f(u);  u' = K + g(·)·dW, g at K (split form) or at u (classic)   [StochasticDiffEq's EM()]
  payoff   max(cp·(S − K), 0), S = exp(x)    src/payoffs/payoffs.jl:154-156, montecarlo.jl:398
  price    discount · mean(payoffs)          src/pricing_methods/montecarlo.jl:489-490
  antithetic pair on −W, pair average        montecarlo.jl:252-263, 431

The state is a value and its Jacobian with respect to the eight seedable scalars SLOTS.  Dual rules, step by step:
  x ± y, x·y                 the sum and product rules
  max(v, 0)                  v and its partials where v > 0, an exact zero with zero partials otherwise
  sqrt(w⁺)                   dw / (2 sqrt w) for w > 0, and 0 at the clip ("Dual rules")
  x0 = log S0                dx0 = dS0 / S0
  exp(x)                     exp(x)·dx
Nothing here restates the device's fused per-step map (hh_sim.h, HestonModel::step): the tests exist to show that
the fused form equals these rules.

Every value and partial carries a running magnitude A, so that ε·A is the size of a first-order forward rounding-error
bound of ANY careful fp64 evaluation of the same quantity, cancellation included.  For a value it is the same
recurrence on absolute values: |x| + |y| for a sum, A_x·A_y for a product, max(|f|, |f'|·A_w) through a function.
For a partial it is the Σ|terms| of the error of its rule: each term of the rule with ONE factor replaced by that
factor's magnitude and the others by their absolute values — for d(xy) = dx·y + x·dy that is A_dx·|y| + |dx|·A_y +
A_x·|dy| + |x|·A_dy, for d√w = dw·g(w) it is A_dw·g + |dw|·|g'|·A_w.  Magnitudes therefore add up along a path as
errors do; they are never multiplied by one another, which would let A outgrow its value by a factor per step.

Every comparison the scheme makes (v > 0, K_v > 0 in the split form, cp·(S_T − K) > 0) is recorded with the compared
quantity and its magnitude.  `reference()` calls a comparison DECIDED when the 50-digit and the fp64 quantity are both
exactly 0, or when the 50-digit |quantity| ≥ 2⁻³⁰·A; a path is USABLE when all its comparisons are decided and the
fp64 run took the same branches.  Only usable paths are compared: on the others a rounding error may legitimately
flip a branch.
"""
import math

import mpmath as mp
import numpy as np

SLOTS = ("S0", "V0", "kappa", "theta", "sigma", "r_drift", "discount", "strike")
NS = len(SLOTS)
EPS = 2.0 ** -52
GUARD = 2.0 ** -30
DPS = 50


def _sqrt(x):
    return math.sqrt(x) if isinstance(x, float) else mp.sqrt(x)


def _exp(x):
    return math.exp(x) if isinstance(x, float) else mp.exp(x)


def _log(x):
    return math.log(x) if isinstance(x, float) else mp.log(x)


class Dual:
    """value v, partials d[NS]; magnitudes a of v and ad[NS] of d"""
    __slots__ = ("v", "d", "a", "ad")

    def __init__(self, v, d, a, ad):
        self.v, self.d, self.a, self.ad = v, d, a, ad

    @classmethod
    def input(cls, v, slot=None):
        z = v - v
        d = [z] * NS
        if slot is not None:
            d[slot] = z + 1
        return cls(v, d, abs(v), list(d))

    def zero(self):
        z = self.v - self.v
        return Dual(z, [z] * NS, z, [z] * NS)

    def __neg__(self):
        return Dual(-self.v, [-x for x in self.d], self.a, self.ad)

    def __add__(self, o):
        if not isinstance(o, Dual):
            return Dual(self.v + o, self.d, self.a + abs(o), self.ad)
        return Dual(self.v + o.v, [x + y for x, y in zip(self.d, o.d)], self.a + o.a,
                    [x + y for x, y in zip(self.ad, o.ad)])

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Dual):
            c = abs(o)
            return Dual(self.v * o, [x * o for x in self.d], self.a * c, [x * c for x in self.ad])
        av, bv = abs(self.v), abs(o.v)
        return Dual(self.v * o.v, [x * o.v + self.v * y for x, y in zip(self.d, o.d)], self.a * o.a,
                    [ax * bv + abs(x) * o.a + av * ay + self.a * abs(y)
                     for x, y, ax, ay in zip(self.d, o.d, self.ad, o.ad)])

    __rmul__ = __mul__


def dlog(x):
    """log of a positive input: partials dx/x"""
    g = 1 / x.v
    return Dual(_log(x.v), [t * g for t in x.d], max(abs(_log(x.v)), x.a * g), [t * g for t in x.ad])


def dexp(x):
    e = _exp(x.v)
    a = e * max(x.a, 1)
    return Dual(e, [e * t for t in x.d], a, [e * at + a * abs(t) for t, at in zip(x.d, x.ad)])


def dmax0(x, record, kind):
    """max(x, 0): the comparison goes on `record`"""
    taken = x.v > 0
    record.append((kind, x.v, x.a, taken))
    return x if taken else x.zero()


def dsqrt_clipped(w):
    """sqrt of a clipped w >= 0 (the comparison w > 0 is dmax0's): tangent dw/(2 sqrt w), 0 at the clip"""
    if not w.v > 0:
        return w.zero()
    s = _sqrt(w.v)
    g = 1 / (2 * s)
    cg = g * w.a / (2 * w.v)  # |dg/dw|·A_w: what w's error does to g
    return Dual(s, [t * g for t in w.d], max(s, w.a * g), [at * g + abs(t) * cg for t, at in zip(w.d, w.ad)])


def _model(case, num):
    p = {name: Dual.input(num(case[name]), i) for i, name in enumerate(SLOTS[:7])}
    p["dt"] = num(case["T"]) / case["n_steps"]
    p["half"] = num(0.5)
    return p


def heston_path(case, p, dW, record):
    """heston.jl:7-16 under EM: f(u) = [μ − max(v,0)/2, κ(Θ − max(v,0))], g(u) = [√max(v,0), σ√max(v,0)]"""
    x, v, dt = dlog(p["S0"]), p["V0"], p["dt"]
    for d1, d2 in dW:
        vp = dmax0(v, record, "v")
        Kx = x + (p["r_drift"] - vp * p["half"]) * dt
        Kv = v + (p["kappa"] * (p["theta"] - vp)) * dt
        sq = dsqrt_clipped(dmax0(Kv, record, "Kv") if case["em_split"] else vp)
        x = Kx + sq * d1
        v = Kv + (p["sigma"] * sq) * d2
    return x


def gbm_path(case, p, dW, record):
    """heston.jl:33-39 under EM: f = μ − σ²/2, g = σ"""
    x, dt = dlog(p["S0"]), p["dt"]
    drift = p["r_drift"] - (p["sigma"] * p["sigma"]) * p["half"]
    for (d1,) in dW:
        x = (x + drift * dt) + p["sigma"] * d1
    return x


def _payoff(x, p, strike, cp, record):
    """payoffs.jl:154-156 on S = exp(x)"""
    S = dexp(x)
    m = (S - strike) * cp
    return S, dmax0(m, record, "itm")


def run(case, num, payoffs):
    """The scheme in the number type of `num` on every path of `case` (increments case["dW"][path][step][comp], taken
    exactly).  -> per path a dict: S [(value, A)] per member, and per payoff (strike, cp): the undiscounted payoff and
    the discounted price contribution (Duals, pair-averaged when antithetic) and the path's comparison records."""
    heston = case["dynamics"] == "heston"
    walk = heston_path if heston else gbm_path
    p = _model(case, num)
    out = []
    for rows in case["dW"]:
        dW = [[num(float(t)) for t in row] for row in rows]
        members = [dW] + ([[[-t for t in row] for row in dW]] if case["antithetic"] else [])
        sim_rec, xs = [], []
        for mdW in members:
            xs.append(walk(case, p, mdW, sim_rec))
        res = dict(sim_record=sim_rec, S=None, payoffs=[])
        for strike, cp in payoffs:
            K = Dual.input(num(strike), NS - 1)
            rec, pays, Ss = [], [], []
            for x in xs:
                S, pay = _payoff(x, p, K, num(cp), rec)
                Ss.append((S.v, S.a))
                pays.append(pay)
            pay = pays[0] if len(pays) == 1 else (pays[0] + pays[1]) * num(0.5)  # montecarlo.jl:431
            res["S"] = Ss
            res["payoffs"].append(dict(payoff=pay, price=p["discount"] * pay, record=rec))
        out.append(res)
    return out


def _decided(q_mp, a_mp, q_64):
    return (q_mp == 0 and q_64 == 0) or abs(q_mp) >= GUARD * a_mp


def _usable(rec_mp, rec_64):
    return all(_decided(qm, am, q6) and tm == t6 for (_, qm, am, tm), (_, q6, _, t6) in zip(rec_mp, rec_64))


def _flat(d):
    return [d.v] + list(d.d)


def _e64(got, want):
    return float(abs(mp.mpf(got) - want))


def reference(case, payoffs, run=run):
    """Both runs of `case` (by `run`: this module's scheme, or another law with the same output, as
    oracle/lognormal_exact.py's) and what the tests need of them.  ->
      n, members         paths, members per path (2 when antithetic)
      S[m][i]            50-digit S_T of member m of path i;  S_e64, S_A: float arrays [m][i]
      clip_fraction      share of (member, step) pairs with v <= 0 (Heston)
      pos_ne_wpos        (member, step) pairs where [v > 0] != [K_v > 0] (split form)
      payoffs[j]         strike, cp, usable[i], and for `payoff` and `price`: `<name>` [i][1 + NS] mpf (value, then
                         the partials in SLOTS order), `<name>_e64`, `<name>_A` float arrays [i][1 + NS]
    e64 = |fp64 run − 50-digit run|; A = the running magnitude of the 50-digit run."""
    with mp.workdps(DPS):
        rm = run(case, mp.mpf, payoffs)
        r6 = run(case, float, payoffs)
        n, members = len(rm), 2 if case["antithetic"] else 1
        sim_ok = np.array([_usable(a["sim_record"], b["sim_record"]) for a, b in zip(rm, r6)])
        vs = [t for a in rm for t in a["sim_record"] if t[0] == "v"]
        ne = 0
        if case["dynamics"] == "heston" and case["em_split"]:
            for a in rm:
                rec = a["sim_record"]
                ne += sum(1 for s, t in zip(rec[0::2], rec[1::2]) if s[3] != t[3])
        ref = dict(n=n, members=members,
                   S=[[a["S"][m][0] for a in rm] for m in range(members)],
                   S_A=np.array([[float(a["S"][m][1]) for a in rm] for m in range(members)]),
                   S_e64=np.array([[_e64(b["S"][m][0], a["S"][m][0]) for a, b in zip(rm, r6)] for m in range(members)]),
                   clip_fraction=(sum(1 for t in vs if not t[3]) / len(vs)) if vs else 0.0,
                   pos_ne_wpos=ne, payoffs=[])
        for j, (strike, cp) in enumerate(payoffs):
            pj = dict(strike=strike, cp=cp)
            pj["usable"] = sim_ok & np.array([_usable(a["payoffs"][j]["record"], b["payoffs"][j]["record"])
                                              for a, b in zip(rm, r6)])
            for name in ("payoff", "price"):
                pj[name] = [_flat(a["payoffs"][j][name]) for a in rm]
                pj[name + "_A"] = np.array([[float(a["payoffs"][j][name].a)] + [float(t) for t in a["payoffs"][j][name].ad]
                                            for a in rm])
                pj[name + "_e64"] = np.array([[_e64(g, w) for g, w in zip(_flat(b["payoffs"][j][name]), row)]
                                              for b, row in zip(r6, pj[name])])
            ref["payoffs"].append(pj)
    return ref
