"""The closed-form lognormal simulations of the reference — the exact terminal law with its forward-mode partials, and
the GBM-process path grid — one primitive at a time, generic in the number type as oracle/euler_exact.py is:
`mpmath.mpf` at 50 digits is the reference the tests hold the device and oracle/hh_oracle.c to, Python `float` is "the
same formulas in fp64" whose distance from the 50-digit run is e64.  TEST INFRASTRUCTURE ONLY.  Dual, its magnitudes,
SLOTS, GUARD, DPS, the payoff rule and the usable-path rule are euler_exact's.

Written from the reference's formulas:
  marginal law   Normal(log S0 + (r − σ²/2)·m, σ·√T)          src/pricing_methods/montecarlo.jl:293-303
                 m = √T as written there (compat_sqrt_alpha), m = T as the lognormal law has it
  sample         x = mean + std·z                              rand(rng, Normal(μ, σ)), montecarlo.jl:412-414
  mirror         2·mean − x                                    montecarlo.jl:386-390
  S = exp x, payoff max(cp·(S − K), 0), pair average, price = discount·mean(payoffs)
                                                               montecarlo.jl:384, 398, 431, 489-490; payoffs.jl:154-156
  grid           W_{k+1} = W_k + W_k·(exp((r − σ²/2)·dt + σ·√dt·z_k) − 1); the antithetic ensemble repeats it with −σ
                 on the same z                                 montecarlo.jl:140-159, 270-284
Nothing here restates hh_sim.h or hh_oracle.c: no law_mu / law_sd pair of constants, no closed-form finish of the
passive directions, no exp(2a)/e for the flipped path.

The partials, by hand, which tests/test_lognormal_exact_host.py evaluates beside the dual rules.  With ℓ = log S0,
s = √T:  x = ℓ + (r − σ²/2)·m + σ·s·z  has  ∂x/∂S0 = 1/S0,  ∂x/∂σ = −σ·m + s·z,  ∂x/∂r = m,  and nothing from V0, κ, θ,
the discount or the strike.  The mirror 2·mean − x = ℓ + (r − σ²/2)·m − σ·s·z has the same ∂/∂S0 and ∂/∂r, and
∂/∂σ = −σ·m − s·z.  In the money the price contribution D·cp·(e^x − K) has ∂/∂p = D·cp·e^x·∂x/∂p for p ∈ {S0, σ, r},
∂/∂D = cp·(e^x − K), ∂/∂K = −D·cp; out of the money everything is an exact zero.

Magnitudes.  The exact law goes through Dual's rules as they stand.  The grid's recursion multiplies two quantities
that BOTH carry accumulated error, W_k and (e − 1): Dual's value rule for a product, A_x·A_y, is meant for a state times
a parameter and would multiply A by 2 + A_e ≥ 3 per date — 3¹⁰⁰ after a hundred, a bar that guards nothing.
euler_exact's own principle ("Σ|terms| of a first-order bound; magnitudes add up along a path as errors do; they are
never multiplied by one another") gives the product the magnitude it gives a partial's product: A_W·|e − 1| +
|W|·A_{e−1}.  So  A_{k+1} = A_k + A_k·|e − 1| + |W_k|·(A_e + 1),  A_e = e·max(A_arg, 1),  A_arg = |r − σ²/2|-magnitude·dt
+ |σ·√dt·z|:  A grows by about 2·|W| per date, as the roundings of a date do.
"""
import math

import mpmath as mp
import numpy as np

from oracle import euler_exact as ex
from oracle.euler_exact import DPS, GUARD, NS, SLOTS, Dual, dexp, dlog  # noqa: F401  (re-exported for the tests)

_S0, _SIGMA, _R, _DISC = (SLOTS.index(s) for s in ("S0", "sigma", "r_drift", "discount"))


def _sqrt(x):
    return math.sqrt(x) if isinstance(x, float) else mp.sqrt(x)


def law_sample(case, num, z):
    """-> (x, mean): the sample of the marginal law on the normal z (a plain number, taken exactly) and the law's mean"""
    S0 = Dual.input(num(case["S0"]), _S0)
    sigma = Dual.input(num(case["sigma"]), _SIGMA)
    r = Dual.input(num(case["r_drift"]), _R)
    T = num(case["T"])
    s = _sqrt(T)
    m = s if case["compat_sqrt_alpha"] else T
    mean = dlog(S0) + (r - (sigma * sigma) * num(0.5)) * m
    std = sigma * s
    return mean + std * z, mean


def run(case, num, payoffs):
    """The exact law in the number type of `num` on every normal of case["z"] — the output of euler_exact.run: per path
    S [(value, A)] per member, per payoff (strike, cp) the undiscounted payoff and the discounted price contribution
    (Duals, pair-averaged when antithetic) and the comparison records."""
    disc = Dual.input(num(case["discount"]), _DISC)
    p = dict(discount=disc)
    out = []
    for zf in case["z"]:
        x, mean = law_sample(case, num, num(zf))  # a double, or a 50-digit normal of the device's generator
        xs = [x] + ([mean * num(2.0) - x] if case["antithetic"] else [])
        res = dict(sim_record=[], S=None, payoffs=[])
        for strike, cp in payoffs:
            K = Dual.input(num(strike), NS - 1)
            rec, pays, Ss = [], [], []
            for xm in xs:
                S, pay = ex._payoff(xm, p, K, num(cp), rec)
                Ss.append((S.v, S.a))
                pays.append(pay)
            pay = pays[0] if len(pays) == 1 else (pays[0] + pays[1]) * num(0.5)  # montecarlo.jl:431
            res["S"] = Ss
            res["payoffs"].append(dict(payoff=pay, price=disc * pay, record=rec))
        out.append(res)
    return out


def reference(case, payoffs):
    """euler_exact.reference of this law: see there.  `case`: S0, sigma, r_drift, discount, T, compat_sqrt_alpha,
    antithetic, z[path]."""
    c = dict(case, dynamics="lognormal-exact-law", em_split=0)
    return ex.reference(c, payoffs, run=run)


# ---- the GBM-process grid ------------------------------------------------------------------------------------------

def grid_run(case, num):
    """-> rows[member][path][k] = (W_k, A_k), k = 0 … n_steps, on case["z"][path][step]; member 1 (antithetic) is −σ"""
    S0, r, T = num(case["S0"]), num(case["r_drift"]), num(case["T"])
    dt = T / case["n_steps"]
    sdt = _sqrt(dt)
    out = []
    for sigma in [num(case["sigma"])] + ([-num(case["sigma"])] if case["antithetic"] else []):
        half = sigma * sigma * num(0.5)
        a, a_mag = (r - half) * dt, (abs(r) + half) * dt
        b = sigma * sdt
        member = []
        for zs in case["z"]:
            W, A = S0, abs(S0)
            rows = [(W, A)]
            for zf in zs:
                z = num(float(zf))
                arg = a + b * z
                e = ex._exp(arg)
                A_e = e * max(a_mag + abs(b * z), 1)
                inc = e - 1
                A = A + A * abs(inc) + abs(W) * (A_e + 1)
                W = W + W * inc
                rows.append((W, A))
            member.append(rows)
        out.append(member)
    return out


def grid_reference(case):
    """-> dict(W[member][path][k] mpf, A and e64 float arrays of that shape)"""
    with mp.workdps(DPS):
        gm, g6 = grid_run(case, mp.mpf), grid_run(case, float)
        return dict(W=[[[w for w, _ in rows] for rows in mem] for mem in gm],
                    A=np.array([[[float(a) for _, a in rows] for rows in mem] for mem in gm]),
                    e64=np.array([[[ex._e64(w6, wm) for (w6, _), (wm, _) in zip(r6, rm)] for r6, rm in zip(m6, mm)]
                                  for m6, mm in zip(g6, gm)]))
