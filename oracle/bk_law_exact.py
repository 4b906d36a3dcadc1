"""The exact conditional law of ∫₀ᵀ V dt given (V₀, V_T) under Heston's variance process, in mpmath — what a
Broadie–Kaya sample is supposed to be drawn from.  TEST INFRASTRUCTURE ONLY.

Written from the paper (Broadie & Kaya 2006, eq. 13) and from nothing else in this repository: no line of csrc/, of
oracle/bk_oracle.py or of the reference's sources was read for it.  With γ(a) = √(κ² − 2σ²ia), ν = 2κθ/σ² − 1:

    ϕ(a) = γ e^{−(γ−κ)T/2} (1 − e^{−κT}) / (κ (1 − e^{−γT}))
           · exp{ (V₀ + V_T)/σ² · [ κ(1 + e^{−κT})/(1 − e^{−κT}) − γ(1 + e^{−γT})/(1 − e^{−γT}) ] }
           · I_ν(z(γ)) / I_ν(z(κ)),           z(g) = √(V₀V_T) · 4g e^{−gT/2} / (σ² (1 − e^{−gT}))

THE BRANCH.  For non-integer ν the ratio of Bessel functions has to be continued continuously in a from a = 0, where it
is 1; the principal branch of I_ν jumps whenever z(γ) crosses the negative real axis, and z(γ) winds around the origin
without end as a grows.  Here the continuation needs no unwrapping: I_ν(z) = z^ν·g(z²) with g entire, so only arg z has
to be carried, and it has a closed form.  z = c·γ·e^{−γT/2}/(1 − e^{−γT}) with c > 0, hence

    arg z = arg γ − Im(γ)·T/2 − arg(1 − e^{−γT}),

and every term is continuous in a: Re γ > 0 for real a (κ² − 2σ²ia lies in the right half-plane, principal root), so
|e^{−γT}| < 1 and 1 − e^{−γT} stays in the right half-plane, where the principal argument is continuous.  At a = 0 the
angle is 0.  g(z²) = I_ν(z)/z^ν is formed from mp.besseli and the principal power at the SAME principal z, whose branch
conventions cancel.  tests/test_bk_law_exact_host.py pins this angle to one carried by continuity on a fine ladder in a.

THE CDF.  F(x) = (2/π) ∫₀^∞ sin(ax)/a · Re ϕ(a) da by the trapezoid rule,
    F_h(x) = hx/π + (2/π) Σ_{j≥1} sin(hjx)/j · Re ϕ(hj),
whose error for a law on [0, ∞) is the aliasing term Σ_k [F(2πk/h + x) − F(2πk/h − x)] ≤ 1 − F(2π/h − x) (Abate & Whitt
1992; Broadie & Kaya eq. 16-17).  The step is chosen from a Chernoff bound P(X > y) ≤ M(s)·e^{−sy}, M(s) = ϕ(−is), so
that the bound is below 10⁻²⁶ for every x up to x_max, and the sum runs until |ϕ| < 10⁻²⁸ three times in a row (|ϕ|
decays like e^{−c√a}: the rest of the sum is then below the last term).  `Law.verify` repeats the sum with half the
step and twice the cut-off.  The density and its derivatives come from the same table of Re ϕ(hj).

THE ALGORITHM'S OWN SERIES.  `alg_series` is the sampler's CDF as the reference states it — moments from central
differences of ϕ with step `moment_h`, h = π/(mean + n_σ·sd), terms until |ϕ(hj)|/j < π·cf_tol/2, the weights of F_h
above — evaluated with the ϕ of this module at 50 digits; `alg_cdf_fp64` is the same, start to end, in numpy/scipy doubles.
"""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

DPS = 40       # the exact law (the issue asks for >= 30)
DPS_ALG = 50   # the algorithm's series
GUARD = 12     # extra digits inside ϕ
ALIAS = mp.mpf(10) ** -26
TAIL = mp.mpf(10) ** -28
VT_FLOOR = 2.0 ** -1000


class Law:
    """ϕ, F, f of ∫V given (V0, VT); every parameter a Python float, taken exactly."""

    def __init__(self, V0, VT, kappa, theta, sigma, T):
        self.par = dict(V0=float(V0), VT=float(VT), kappa=float(kappa), theta=float(theta), sigma=float(sigma), T=float(T))
        self.table = None

    # ---- the characteristic function ---------------------------------------------------------------------------------
    def _consts(self):
        p = self.par
        k, T = mp.mpf(p["kappa"]), mp.mpf(p["T"])
        s2 = mp.mpf(p["sigma"]) ** 2
        V0, VT = mp.mpf(p["V0"]), mp.mpf(p["VT"])
        nu = 2 * k * mp.mpf(p["theta"]) / s2 - 1
        return k, T, s2, V0, VT, nu

    @staticmethod
    def _g(nu, z):
        """I_ν(z)/z^ν, entire in z² (both factors on the principal branch of the same z)"""
        return mp.besseli(nu, z) / mp.power(z, nu)

    def angle(self, a):
        """the continuous argument of z(γ(a)), 0 at a = 0"""
        k, T, s2, *_ = self._consts()
        g = mp.sqrt(k * k - 2 * s2 * mp.mpc(0, 1) * a)
        return mp.arg(g) - mp.im(g) * T / 2 - mp.arg(-mp.expm1(-g * T))

    def z(self, a):
        """the principal z(γ(a)) (for the ladder test of the angle)"""
        k, T, s2, V0, VT, _ = self._consts()
        g = mp.sqrt(k * k - 2 * s2 * mp.mpc(0, 1) * a)
        return 4 * mp.sqrt(V0 * VT) / s2 * g * mp.exp(-g * T / 2) / (-mp.expm1(-g * T))

    def phi(self, a):
        with mp.workdps(mp.mp.dps + GUARD):
            k, T, s2, V0, VT, nu = self._consts()
            g = mp.sqrt(k * k - 2 * s2 * mp.mpc(0, 1) * a)
            dk, dg = -mp.expm1(-k * T), -mp.expm1(-g * T)          # 1 − e^{−κT}, 1 − e^{−γT}
            first = g * mp.exp(-(g - k) * T / 2) * dk / (k * dg)
            second = mp.exp((V0 + VT) / s2 * (k * (2 - dk) / dk - g * (2 - dg) / dg))
            c = 4 * mp.sqrt(V0 * VT) / s2
            zk = c * k * mp.exp(-k * T / 2) / dk
            zg = c * g * mp.exp(-g * T / 2) / dg
            theta = mp.arg(g) - mp.im(g) * T / 2 - mp.arg(dg)
            ratio = mp.exp(nu * mp.mpc(mp.log(abs(zg) / zk), theta)) * self._g(nu, zg) / self._g(nu, zk)
            out = first * second * ratio
        return +out

    def mgf(self, s):
        """E exp(s·∫V) = ϕ(−is), finite for s < (κ² + 4π²/T²)/(2σ²)"""
        return mp.re(self.phi(mp.mpc(0, -1) * s))

    def moments(self):
        """(mean, variance) from the cumulant function log M(s) by 50-digit central differences"""
        with mp.workdps(60):
            d = mp.mpf(10) ** -12
            lp, lm = mp.log(self.mgf(d)), mp.log(self.mgf(-d))
            return (lp - lm) / (2 * d), (lp + lm) / (d * d)

    # ---- the table of Re ϕ(hj) ---------------------------------------------------------------------------------------
    def step_for(self, x_max):
        """the largest step whose aliasing term is below ALIAS for every x <= x_max: 2π/h − x_max >= y with
        M(s)·e^{−sy} <= ALIAS, the best of a few s below the mgf's pole"""
        k, T, s2, *_ = self._consts()
        s_pole = (k * k + 4 * mp.pi ** 2 / (T * T)) / (2 * s2)
        y = min((mp.log(self.mgf(q * s_pole)) - mp.log(ALIAS)) / (q * s_pole) for q in (0.3, 0.5, 0.7, 0.85, 0.95))
        return 2 * mp.pi / (y + x_max)

    def _sum_terms(self, h, offset, a_stop=None):
        """Re ϕ(h·(j − offset)), j = 1, 2, …: until |ϕ| < TAIL three times in a row, or (a_stop) up to a_stop"""
        out, small, j = [], 0, 1
        while True:
            a = h * (j - offset)
            if a_stop is not None and a > a_stop:
                break
            v = self.phi(a)
            out.append(mp.re(v))
            if a_stop is None:
                small = small + 1 if abs(v) < TAIL else 0
                if small == 3:
                    break
            j += 1
        return out

    def build(self, x_max):
        h = self.step_for(x_max)
        self.table = dict(h=h, re=self._sum_terms(h, 0), x_max=mp.mpf(x_max))
        return self

    @staticmethod
    def _series(h, re, x, kind, offset=0):
        """kind 0: Σ sin(ax)/a·Re ϕ·h (F's sum), 1: Σ cos(ax)·Re ϕ·h (f), n >= 2: its (n−1)-th derivative;
        a = h·(j − offset).  sin and cos by the recurrence of e^{iax}."""
        w, cur = mp.expj(h * x), mp.expj(h * x * (1 - offset))
        tot = mp.mpf(0)
        for j, r in enumerate(re, start=1):
            a = h * (j - offset)
            if kind == 0:
                tot += mp.im(cur) / a * r
            else:
                n = kind - 1  # d^n/dx^n cos(ax) = a^n cos(ax + nπ/2)
                trig = (mp.re(cur), -mp.im(cur), -mp.re(cur), mp.im(cur))[n % 4]
                tot += a ** n * trig * r
            cur *= w
        return 2 / mp.pi * h * tot

    def F(self, x):
        t = self.table
        with mp.workdps(mp.mp.dps + GUARD):
            out = t["h"] * x / mp.pi + self._series(t["h"], t["re"], mp.mpf(x), 0)
        return +out

    def pdf(self, x, order=0):
        """f(x) = (2/π) ∫₀^∞ cos(ax) Re ϕ(a) da (the a = 0 term of the trapezoid rule has weight 1/2), or its
        order-th derivative"""
        t = self.table
        with mp.workdps(mp.mp.dps + GUARD):
            out = self._series(t["h"], t["re"], mp.mpf(x), 1 + order) + (t["h"] / mp.pi if order == 0 else 0)
        return +out

    def derivative_bound(self, order):
        """sup over x of |d^order f/dx^order| <= (2/π) ∫₀^∞ a^order |Re ϕ(a)| da, from the table"""
        t = self.table
        return 2 / mp.pi * t["h"] * mp.fsum((t["h"] * j) ** order * abs(r) for j, r in enumerate(t["re"], start=1))

    def verify(self, xs):
        """F by half the step and twice the cut-off against F of the table, at every x of xs -> the largest difference.
        (The half step's even points are the table's own; its odd points and everything between the table's end and
        twice that are evaluated anew.)"""
        t = self.table
        h, re = t["h"], t["re"]
        a_end = h * len(re)
        odd = self._sum_terms(h, mp.mpf(1) / 2, a_stop=2 * a_end)
        beyond = self._sum_terms(h, -len(re), a_stop=2 * a_end)  # a = h·(N + j) up to 2·a_end
        worst = mp.mpf(0)
        for x in xs:
            x = mp.mpf(x)
            with mp.workdps(mp.mp.dps + GUARD):
                even = self._series(h, re + beyond, x, 0)
                fine = h * x / (2 * mp.pi) + (even + self._series(h, odd, x, 0, mp.mpf(1) / 2)) / 2
            worst = max(worst, abs(fine - self.F(x)))
        return worst

    def quantile(self, u, x0):
        """x* with F(x*) = u, Newton from x0 (mp.findroot with the density as derivative)"""
        u = mp.mpf(u)
        return mp.findroot(lambda x: self.F(x) - u, mp.mpf(x0), solver="newton", df=self.pdf,
                           tol=mp.mpf(10) ** -30, maxsteps=20)

    def table_fp64(self):
        t = self.table
        return float(t["h"]), np.array([float(r) for r in t["re"]])


def cdf_fp64(h, re, x):
    """F of a table in doubles (a start for the Newton iteration, nothing more)"""
    j = np.arange(1, len(re) + 1, dtype=np.float64)
    return h * x / math.pi + 2 / math.pi * float(np.sum(np.sin(h * j * x) / j * re))


def start_of(law, u, lo, hi):
    """a double near F⁻¹(u) by bisection on the fp64 table between lo and hi"""
    h, re = law.table_fp64()
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if cdf_fp64(h, re, mid) < u:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-13 * hi:
            break
    return 0.5 * (lo + hi)


# ---- the sampler's own series ------------------------------------------------------------------------------------------

def alg_setup(law, n_sigma, moment_h):
    """(mean, sd², h) as the sampler forms them: central differences of ϕ with step moment_h, variance floored at
    10⁻¹², h = π/(mean + n_σ·sd)"""
    d = mp.mpf(moment_h)
    pp, p0, pm = law.phi(d), law.phi(mp.mpf(0)), law.phi(-d)
    mean = mp.re(-mp.mpc(0, 1) * (pp - pm) / (2 * d))
    var = mp.re(-(pp - 2 * p0 + pm) / (d * d)) - mean * mean
    s2 = max(var, mp.mpf(10) ** -12)
    return mean, s2, mp.pi / (mean + mp.mpf(n_sigma) * mp.sqrt(s2))


def alg_series(law, n_sigma, cf_tol, moment_h, max_terms=200000):
    """-> dict(h, re[], mean, s2): the terms j = 1 … N of the sampler's CDF series, N the first j with
    |ϕ(hj)|/j < π·cf_tol/2 (that term included), at DPS_ALG digits"""
    with mp.workdps(DPS_ALG):
        mean, s2, h = alg_setup(law, n_sigma, moment_h)
        bound = mp.pi * mp.mpf(cf_tol) / 2
        re = []
        for j in range(1, max_terms + 1):
            v = law.phi(h * j)
            re.append(mp.re(v))
            if abs(v) / j < bound:
                break
        else:
            raise ArithmeticError("the sampler's series did not stop")
        return dict(h=h, re=re, mean=mean, s2=s2)


def alg_cdf(series, x):
    with mp.workdps(DPS_ALG):
        x = mp.mpf(x)
        return +(series["h"] * x / mp.pi + Law._series(series["h"], series["re"], x, 0))


def phi_fp64(par, a):
    """ϕ in numpy/scipy doubles, by the formulas of Law.phi (scaled Bessel function; a an array)"""
    from scipy import special
    k, T, s2 = par["kappa"], par["T"], par["sigma"] ** 2
    V0, VT = par["V0"], par["VT"]
    nu = 2 * k * par["theta"] / s2 - 1
    a = np.asarray(a, dtype=np.float64)
    g = np.sqrt(k * k - 2j * s2 * a)
    dk, dg = -np.expm1(-k * T), -np.expm1(-g * T)
    first = g * np.exp(-(g - k) * T / 2) * dk / (k * dg)
    second = np.exp((V0 + VT) / s2 * (k * (2 - dk) / dk - g * (2 - dg) / dg))
    c = 4 * math.sqrt(V0) * math.sqrt(VT) / s2
    zk = c * k * math.exp(-k * T / 2) / dk
    zg = c * g * np.exp(-g * T / 2) / dg
    theta = np.angle(g) - g.imag * T / 2 - np.angle(dg)
    if zk < 1e-100:  # the absorbed variance: I_ν(z) = (z/2)^ν/Γ(ν+1) to every digit
        ratio = np.exp(nu * (np.log(np.abs(zg) / zk) + 1j * theta))
    else:
        # I_ν(z)/z^ν at the principal z, with the factor e^{|Re z|} of the scaled function put back
        lg = np.log(special.ive(nu, zg)) + np.abs(zg.real) - nu * np.log(zg)
        lk = math.log(special.ive(nu, zk)) + zk - nu * math.log(zk)
        ratio = np.exp(nu * (np.log(np.abs(zg) / zk) + 1j * theta) + lg - lk)
    return first * second * ratio


def alg_cdf_fp64(par, x, n_sigma, cf_tol, moment_h, block=64):
    """the sampler's CDF at x, start to end in doubles: its moments, its h, its stopping rule, its sum"""
    pp, p0, pm = phi_fp64(par, [moment_h, 0.0, -moment_h])
    mean = ((pp - pm) / (2 * moment_h) * -1j).real
    var = (-(pp - 2 * p0 + pm) / moment_h ** 2).real - mean * mean
    h = math.pi / (mean + n_sigma * math.sqrt(max(var, 1e-12)))
    total, j0 = h * x / math.pi, 1
    while j0 < 10 ** 7:
        j = np.arange(j0, j0 + block, dtype=np.float64)
        v = phi_fp64(par, h * j)
        stop = np.abs(v) / j < math.pi * cf_tol / 2
        n = int(np.argmax(stop)) + 1 if stop.any() else block
        total += 2 / math.pi * float(np.sum(np.sin(h * j[:n] * x) / j[:n] * v[:n].real))
        if stop.any():
            return total, j0 - 1 + n
        j0 += block
    raise ArithmeticError("the sampler's series did not stop")
