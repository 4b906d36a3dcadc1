"""The truncated Carr–Madan integral to 40+ digits (mpmath): the exact value the device quadrature of
hedgehog.jl_amd/csrc/hh_fourier.hip is tested against (tests/golden/carr_madan_exact.json).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tests/golden/make_carr_madan_exact.py, never by the
product, and it imports nothing from the product.  Every formula below is written out from the
mathematics it states; nothing is taken from another implementation.

What is computed
----------------
For a log-price law with characteristic function ϕ(u) = E exp(iu·log S_T), damping α > 0 and bound B,

    call(K) = Re ∫_{-B}^{B} f(v) dv,
    f(v)    = e^{-α log K}/(2π) · D·ϕ(v − i(α+1)) / (α² + α − v² + i v(2α+1)) · e^{-i v log K},

which is the damped-call transform of Carr and Madan (1999) cut off at ±B: the quantity the method
of the modelled project integrates (carr_madan.jl:47-92), *including* its truncation error.  D is the
discount factor, passed separately from the drift rate because the entry points take them separately.

Derived (not measured):

* Evenness.  ϕ(−conj u) = conj ϕ(u) for any law, the denominator and the phase have the same symmetry
  under v -> −v, so f(−v) = conj f(v) and Re ∫_{-B}^{B} f = 2 Re ∫_0^B f.  Only [0, B] is integrated.
* The singularities of f.  The denominator is −(v − iα)(v + i(α+1)): a pole at v = iα, at distance α from
  the real line, with residue ∝ ϕ(−i)·D — the discounted forward, S0 when drift and discount agree —
  whatever the model, strike and expiry.  This is what a Gauss–Legendre panel next to v = 0 has to
  resolve, and why the sub-intervals below are graded down to width α at v = 0 (mpmath's quadrature then
  converges geometrically on each: the pole is ≥ 2.2 half-widths from every sub-interval's centre).
* The laws.  Normal(μ, s) for log S_T: ϕ(t) = exp(iμt − s²t²/2), with s = σ√T and μ = log S0 +
  (r − σ²/2)·T — or ·√T where the modelled project's marginal law has it (`compat_sqrt_alpha`), the two
  agreeing at T = 1 only.  Heston (1993) in the formulation of Albrecher et al. (2007) with exp(−d₁T):
      d₁ = sqrt((κ − ρσ·iu)² + σ²(iu + u²)),  g = (κ − ρσ·iu − d₁)/(κ − ρσ·iu + d₁),
      C = κθ/σ² · [(κ − ρσ·iu − d₁)T − 2·L],   L = log((1 − g e^{−d₁T})/(1 − g)),
      D_v = (κ − ρσ·iu − d₁)/σ² · (1 − e^{−d₁T})/(1 − g e^{−d₁T}),
      ϕ(u) = exp(C + D_v·V0 + iu(log S0 + rT)).
* The logarithm L by continuity.  log ϕ is analytic along Im u = −(α+1) as long as the (α+1)-th moment
  of S_T is finite, so the right L is the continuous one.  At v = 0, iu = α+1 is real; when
  (κ − ρσ(α+1))² ≥ σ²α(α+1) and κ − ρσ(α+1) > 0, d₁ ≥ 0 and 0 ≤ g < 1 are real, the argument of the
  logarithm is a positive real and L is real: the (α+1)-th moment then exists for every T
  (`moment_exists_for_all_T`).  Otherwise d₁ = ib is imaginary at v = 0, g = e^{−2iφ} with φ =
  atan2(b, κ − ρσ(α+1)), the argument is e^{−ibT/2}·sin(φ + bT/2)/sin φ, and the moment is finite exactly
  while φ + bT/2 < π (`moment_exists_at`); Im L = −bT/2 there, the principal value when bT/2 < π.  From
  that anchor L is continued along v on a grid of spacing `ANCHOR_STEP`; between neighbouring anchors its
  argument may not move by more than 1 rad (asserted), so at any quadrature node the sheet nearest the
  closest anchor is the continuous one.  `UnwrappedLog.max_sheet` is the largest |n| of 2πi·n that the
  continuation ever added to the principal value: 0 means the principal branch — what the device takes —
  is the continuous one on the whole line.  By the evenness above the same holds on v < 0.
* Puts by parity on the truncated call, as the entry points do: put = call − S0 + K·D.
* The gradient.  The call as a function of (S0, V0, κ, θ, σ, ρ, r_drift, D) — the eight slots of
  enum hh_cm_grad, drift and discount independent — differentiated by central differences with relative
  step 1e-14 at `DPS` digits: truncation ~ step² · f‴/6 ≤ 1e-27 relative for the O(1)-conditioned
  parameters used, rounding ~ 10^(−DPS)/step.

Measured (by tests/test_carr_madan_exact_host.py, not proven here): that the result equals the closed
lognormal price where the truncated tail is below 1e-30, an independent Gil-Pelaez Heston price, and
that `max_sheet` is 0 on every golden case.
"""
from __future__ import annotations

import mpmath as mp

DPS = 50            # working digits (the golden file keeps 30)
ANCHOR_STEP = mp.mpf(1) / 8
GRAD_SLOTS = ("S0", "V0", "kappa", "theta", "sigma", "rho", "r_drift", "discount")


def _mpf(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(x)  # a Python float converts exactly


def moment_exists_for_all_T(kappa, sigma, rho, alpha) -> bool:
    k = _mpf(kappa) - _mpf(rho) * _mpf(sigma) * (_mpf(alpha) + 1)
    return bool(k > 0 and k * k >= _mpf(sigma) ** 2 * _mpf(alpha) * (_mpf(alpha) + 1))


def moment_exists_at(kappa, sigma, rho, alpha, T) -> bool:
    """E S_T^(α+1) < ∞ (Andersen–Piterbarg 2007, restated in the module docstring)."""
    if moment_exists_for_all_T(kappa, sigma, rho, alpha):
        return True
    a1 = _mpf(alpha) + 1
    k = _mpf(kappa) - _mpf(rho) * _mpf(sigma) * a1
    b2 = _mpf(sigma) ** 2 * _mpf(alpha) * a1 - k * k
    if b2 <= 0:  # k <= 0 with a real d1: the moment explodes at T* = log((k−d)/(k+d))/d
        d = mp.sqrt(-b2)
        return bool(_mpf(T) < mp.log((k - d) / (k + d)) / d) if d > 0 else bool(_mpf(T) < -2 / k)
    b = mp.sqrt(b2)
    return bool(mp.atan2(b, k) + b * _mpf(T) / 2 < mp.pi)


class UnwrappedLog:
    """L(v) = log((1 − g e^{−d₁T})/(1 − g)) on Im u = −(α+1), continued from v = 0 (module docstring)."""

    def __init__(self, p, bound):
        self.p = p
        self.max_sheet = 0
        n = int(mp.ceil(_mpf(bound) / ANCHOR_STEP)) + 1
        u0 = mp.mpc(0, -(p["alpha"] + 1))
        z0, d0 = _heston_parts(p, u0)[3], _heston_parts(p, u0)[1]
        # the anchor: Im L(0) = −Im(d₁)·T/2 (0 for a real d₁), which the principal value gives
        assert abs(mp.arg(z0) + d0.imag * p["T"] / 2) < mp.mpf(10) ** (-DPS + 10), "v = 0: not the principal value"
        self.anchor = [mp.arg(z0)]
        for j in range(1, n + 1):
            a = mp.arg(self._arg_of(j * ANCHOR_STEP))
            prev = self.anchor[-1]
            a += 2 * mp.pi * mp.nint((prev - a) / (2 * mp.pi))
            assert abs(a - prev) < 1, "the anchors are too coarse to continue the logarithm"
            self.anchor.append(a)

    def _arg_of(self, v):
        return _heston_parts(self.p, mp.mpc(v, -(self.p["alpha"] + 1)))[3]

    def __call__(self, v, z):
        """log z for z = the logarithm's argument at real v >= 0, on the continuous sheet."""
        j = int(mp.nint(v / ANCHOR_STEP))
        pr = mp.log(z)
        n = int(mp.nint((self.anchor[min(j, len(self.anchor) - 1)] - pr.imag) / (2 * mp.pi)))
        self.max_sheet = max(self.max_sheet, abs(n))
        return pr + mp.mpc(0, 2 * mp.pi * n)


def _heston_parts(p, u):
    iu = mp.mpc(0, 1) * u
    kri = p["kappa"] - p["rho"] * p["sigma"] * iu
    d1 = mp.sqrt(kri * kri + p["sigma"] ** 2 * (iu + u * u))
    g = (kri - d1) / (kri + d1)
    ed = mp.exp(-d1 * p["T"])
    return kri, d1, ed, (1 - g * ed) / (1 - g), g


def heston_log_cf(p, u, log_fn):
    kri, d1, ed, z, g = _heston_parts(p, u)
    s2 = p["sigma"] ** 2
    C = p["kappa"] * p["theta"] / s2 * ((kri - d1) * p["T"] - 2 * log_fn(z))
    Dv = (kri - d1) / s2 * (1 - ed) / (1 - g * ed)
    return C + Dv * p["V0"] + mp.mpc(0, 1) * u * (mp.log(p["S0"]) + p["r_drift"] * p["T"])


def normal_log_cf(p, t):
    sq = mp.sqrt(p["T"])
    mu = mp.log(p["S0"]) + (p["r_drift"] - p["sigma"] ** 2 / 2) * (sq if p["compat_sqrt_alpha"] else p["T"])
    return mp.mpc(0, 1) * t * mu - (p["sigma"] * sq) ** 2 * t * t / 2


def _breakpoints(alpha, bound):
    """[0, bound] cut into sub-intervals no wider than 2, graded down to width α at v = 0."""
    pts, w = [mp.mpf(0)], min(_mpf(alpha), mp.mpf(2))
    while pts[-1] < bound:
        pts.append(min(pts[-1] + w, _mpf(bound)))
        w = min(2 * w, mp.mpf(2))
    return pts


def _params(case):
    p = {k: _mpf(case[k]) for k in ("S0", "K", "T", "r_drift", "discount", "alpha", "bound", "sigma")}
    p["dynamics"] = case["dynamics"]
    if case["dynamics"] == "heston":
        p.update({k: _mpf(case[k]) for k in ("V0", "kappa", "theta", "rho")})
    else:
        p["compat_sqrt_alpha"] = bool(case.get("compat_sqrt_alpha", False))
    return p


def call_price(case, info=None):
    """The truncated Carr–Madan call of `case` (a dict of floats or mpf; see tests/golden/
    make_carr_madan_exact.py for the keys).  info, if a dict, receives `max_sheet` for Heston."""
    with mp.workdps(DPS):
        p = _params(case)
        logK, alpha = mp.log(p["K"]), p["alpha"]
        if p["dynamics"] == "heston":
            assert moment_exists_at(p["kappa"], p["sigma"], p["rho"], alpha, p["T"]), "no (α+1)-th moment"
            unwrapped = UnwrappedLog(p, p["bound"])
            log_cf = lambda v: heston_log_cf(p, mp.mpc(v, -(alpha + 1)), lambda z: unwrapped(v, z))
        else:
            unwrapped = None
            log_cf = lambda v: normal_log_cf(p, mp.mpc(v, -(alpha + 1)))

        def f(v):
            den = alpha * alpha + alpha - v * v + mp.mpc(0, 1) * v * (2 * alpha + 1)
            return (mp.exp(log_cf(v) - mp.mpc(0, 1) * v * logK) / den).real

        pts = _breakpoints(alpha, p["bound"])
        total = mp.fsum(mp.quad(f, [a, b], method="gauss-legendre") for a, b in zip(pts, pts[1:]))
        if info is not None and unwrapped is not None:
            info["max_sheet"] = unwrapped.max_sheet
        return +(2 * total * p["discount"] * mp.exp(-alpha * logK) / (2 * mp.pi))


def price(case, info=None):
    """Call, or put by parity on the truncated call (cp = −1)."""
    with mp.workdps(DPS):
        c = call_price(case, info)
        return c if case.get("cp", 1.0) > 0 else c - _mpf(case["S0"]) + _mpf(case["K"]) * _mpf(case["discount"])


def shifted(case, name, sign, rel_step="1e-14"):
    """-> (`case` with parameter `name` moved by sign·h, h), h = rel_step·|x| (rel_step itself at x = 0)."""
    with mp.workdps(DPS):
        x = _mpf(case[name])
        h = mp.mpf(rel_step) * (abs(x) if x != 0 else 1)
        return {**case, name: x + sign * h}, h


def call_gradient(case):
    """∂call/∂(S0, V0, κ, θ, σ, ρ, r_drift, discount) by central differences at DPS digits; the slots a
    law does not have (lognormal: V0, κ, θ, ρ) are 0."""
    with mp.workdps(DPS):
        out = []
        for name in GRAD_SLOTS:
            if name not in case:
                out.append(mp.mpf(0))
                continue
            (up, h), (dn, _) = shifted(case, name, +1), shifted(case, name, -1)
            out.append((call_price(up) - call_price(dn)) / (2 * h))
        return out
