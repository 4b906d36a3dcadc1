"""The device Carr–Madan rule restated in numpy complex128 (hedgehog.jl_amd/csrc/hh_fourier.hip): the same
formulas, the same 256 panels × m sub-panels × 16-point Gauss–Legendre, evaluated on the CPU.

TEST INFRASTRUCTURE ONLY.  Two uses: `fixed_rule(case, m)` is what a given sub-panel count computes
(m = 1: the plain 256-panel rule), and `converged(case)` is the same formulas on rules fine enough that
doubling them changes nothing above 1e-15·S0 (or above fp64 rounding, see `converged`) — their distance from
the exact integral (oracle/carr_madan_exact.py) is fp64 rounding alone, the `e64` of
tests/golden/carr_madan_exact.json.  The gradient carries (κ, σ, ρ) partials through the CF as the device
does; the other slots are linear in log ϕ.
"""
from __future__ import annotations

import math

import numpy as np

_GLX, _GLW = np.polynomial.legendre.leggauss(16)
PANELS = 256
SUBPANEL_C = 0.75   # the kernel's rule: bound/(256·m) <= 0.75·alpha


def subpanels(alpha, bound):
    return max(1, math.ceil(bound / (PANELS * SUBPANEL_C * alpha)))


class _Z:
    """complex128 arrays with partials along (κ, σ, ρ)."""
    __slots__ = ("v", "d")
    __array_ufunc__ = None   # ndarray ∘ _Z defers to _Z's reflected operators

    def __init__(self, v, d=None):
        self.v = v
        self.d = d if d is not None else [0.0, 0.0, 0.0]

    @staticmethod
    def lift(x):
        return x if isinstance(x, _Z) else _Z(x)

    def __add__(self, o):
        o = _Z.lift(o)
        return _Z(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])
    __radd__ = __add__

    def __sub__(self, o):
        o = _Z.lift(o)
        return _Z(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

    def __rsub__(self, o):
        return _Z.lift(o) - self

    def __mul__(self, o):
        o = _Z.lift(o)
        return _Z(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _Z.lift(o)
        q = self.v / o.v
        return _Z(q, [(a - q * b) / o.v for a, b in zip(self.d, o.d)])

    def sqrt(self):
        r = np.sqrt(self.v)
        return _Z(r, [a / (2 * r) for a in self.d])

    def exp(self):
        r = np.exp(self.v)
        return _Z(r, [r * a for a in self.d])

    def log(self):
        return _Z(np.log(self.v), [a / self.v for a in self.d])


def _heston_CD(c, u):
    kappa, sigma, rho = _Z(c["kappa"], [1.0, 0.0, 0.0]), _Z(c["sigma"], [0.0, 1.0, 0.0]), _Z(c["rho"], [0.0, 0.0, 1.0])
    iu = 1j * u
    kri = kappa - iu * (rho * sigma)
    s2 = sigma * sigma
    d1 = (kri * kri + (iu + u * u) * s2).sqrt()
    g = (kri - d1) / (kri + d1)
    ed = (-c["T"] * d1).exp()
    one_m_ged = 1.0 - g * ed
    C = c["theta"] * ((kappa / s2) * (c["T"] * (kri - d1) - 2.0 * (one_m_ged / (1.0 - g)).log()))
    Dv = ((kri - d1) * ((1.0 - ed) / one_m_ged)) / s2
    return C, Dv


def _nodes(bound, panels):
    """Panel centres as the kernel forms them: −bound + (k + ½)·w for the plain 256 panels, and (2k + 1 − panels)·h
    — an exact integer times h, so that a centre next to v = 0 is not rounded at the size of the bound — beyond."""
    h = bound / panels
    k = np.arange(panels)
    mid = -bound + (k + 0.5) * (2.0 * bound / PANELS) if panels == PANELS else (2 * k + 1 - panels).astype(np.float64) * h
    return (mid[:, None] + h * _GLX[None, :]).ravel(), np.tile(_GLW * h, panels)


def rule(c, panels, grad=False):
    """The call of `c` (and its 8 partials) on `panels` equal Gauss–Legendre panels over (−bound, bound)."""
    v, w = _nodes(c["bound"], panels)
    alpha, logK = c["alpha"], math.log(c["K"])
    u = v - 1j * (alpha + 1.0)
    iu = 1j * u
    den = alpha * alpha + alpha - v * v + 1j * v * (2.0 * alpha + 1.0)
    kern = w * (math.exp(-alpha * logK) / (2 * math.pi) * c["discount"]) / den * np.exp(-1j * v * logK)
    dl = [0.0] * 7
    if c["dynamics"] == "heston":
        C, Dv = _heston_CD(c, u)
        phi = np.exp(C.v + c["V0"] * Dv.v + (math.log(c["S0"]) + c["r_drift"] * c["T"]) * iu)
        dl = [iu / c["S0"], Dv.v, C.d[0] + c["V0"] * Dv.d[0], C.v / c["theta"], C.d[1] + c["V0"] * Dv.d[1],
              C.d[2] + c["V0"] * Dv.d[2], c["T"] * iu]
    else:
        sq = math.sqrt(c["T"])
        tmul = sq if c.get("compat_sqrt_alpha") else c["T"]
        mu, sd = math.log(c["S0"]) + (c["r_drift"] - 0.5 * c["sigma"] ** 2) * tmul, c["sigma"] * sq
        phi = np.exp(mu * iu - (0.5 * sd * sd) * (u * u))
        dl[0], dl[4], dl[6] = iu / c["S0"], (-c["sigma"] * tmul) * iu - (c["sigma"] * c["T"]) * (u * u), tmul * iu
    base = kern * phi
    call = math.fsum(base.real)
    if not grad:
        return call
    g = [math.fsum((base * d).real) if not isinstance(d, float) else 0.0 for d in dl]
    return call, np.array(g + [call / c["discount"]])


def fixed_rule(c, m=1, grad=False):
    """256 panels, each in m equal sub-panels — the same nodes as 256·m equal panels."""
    return rule(c, PANELS * m, grad)


def converged(c, grad=False):
    """The rule on 2, 4 and 8 times the kernel's sub-panel count: -> (the three results, the largest move from
    one to the next relative to S0 — and, with the gradient, to each partial's scale S0/max(|x|, 0.05)).  The
    pole's contribution is gone from the first on (it falls by ~1e-10 per halving at these widths), so what
    still moves is fp64 rounding: below 1e-15 wherever nothing cancels (tests/test_carr_madan_exact_host.py
    holds the golden cases to that), up to 1e-12 at vol of vol 0.001 (asserted here).  Three samples of that
    rounding rather than one: `e64` is the worst of them."""
    m = subpanels(c["alpha"], c["bound"])
    res = [rule(c, PANELS * m * k, grad) for k in (2, 4, 8)]
    if not grad:
        move = max(abs(a - b) for a, b in zip(res, res[1:])) / c["S0"]
    else:
        move = max(max(abs(a[0] - b[0]) / c["S0"], float(np.max(np.abs(a[1] - b[1]) / grad_scales(c))))
                   for a, b in zip(res, res[1:]))
    assert move <= 1e-12, "the fp64 rule does not settle"
    return res, move


GRAD_SLOTS = ("S0", "V0", "kappa", "theta", "sigma", "rho", "r_drift", "discount")


def grad_scales(c, grad=None):
    """scale = max(|∂|, S0/max(|x|, 0.05)) per slot (|∂| left out when grad is None)."""
    s = np.array([c["S0"] / max(abs(c.get(n, 0.0)), 0.05) for n in GRAD_SLOTS])
    return s if grad is None else np.maximum(s, np.abs(np.asarray(grad, dtype=np.float64)))
