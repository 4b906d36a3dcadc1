"""The Carr–Madan rule under the laws with a jump or a gamma clock (Merton, Bates, Variance Gamma), stated once.

Part 1, the frame: what tests/merton_cases.py, tests/bates_cases.py and tests/vg_cases.py share when they restate the
truncated Carr–Madan call — exactly (mpmath, on oracle/carr_madan_exact.py's graded breakpoints) and as the device's rule
(numpy complex128, on oracle/carr_madan_fp64.py's nodes).  A law brings two functions:
  log_cf(case) -> f(v)      log ϕ(v − i(α+1)) in mpmath, v real
  phi(case, u) -> array     ϕ(u) in complex128, in hh_fourier.hip's own expressions and operand order

Part 2, the pins: the Carr–Madan entry points of the C-ABI BIT FOR BIT — what tests/golden/make_carr_madan_pins.py
records and tests/test_gpu_carr_madan_pins.py recomputes.  Every case is one call with one or three payoffs; its pin is
the SHA-256 of the returned doubles.  Rules: α = 1, bound 32 (one sub-panel per lane, centred at the plain rule's `mid`)
and α = 0.5, bound 1000 (⌈1000/96⌉ = 11 sub-panels, centred at integer multiples of the half-width).  The basket of three
holds a call and a put, two expiries and two rates: several workgroups, the per-payoff law quantities and the parity line.
Every input is a literal double, so that no library's exp or log stands between the fixture and the entry point.
"""
import ctypes as C
import hashlib
import json
import math
import os
import shutil
import subprocess

import mpmath as mp
import numpy as np

from oracle import carr_madan_exact as cx
from oracle import carr_madan_fp64 as fp
from oracle import euler_exact as ex

DPS = ex.DPS


# ---- 1. the frame ---------------------------------------------------------------------------------------------------------

def cm_case(c, K, alpha, bound, cp=1.0):
    """a model and a payoff in the form the functions below take"""
    return dict(c, K=K, alpha=alpha, bound=bound, cp=cp, discount=c.get("discount", math.exp(-c["r_drift"] * c["T"])))


def cm_exact_call(case, log_cf):
    """The truncated Carr–Madan call of `case` under the law of log_cf, exactly integrated: oracle/carr_madan_exact.py's
    integrand on its graded sub-intervals of [0, bound] (the integrand's real part is even: twice the half)."""
    with mp.workdps(DPS):
        alpha, logK = cx._mpf(case["alpha"]), mp.log(cx._mpf(case["K"]))
        lcf = log_cf(case)

        def f(v):
            den = alpha * alpha + alpha - v * v + mp.mpc(0, 1) * v * (2 * alpha + 1)
            return (mp.exp(lcf(v) - mp.mpc(0, 1) * v * logK) / den).real

        pts = cx._breakpoints(alpha, cx._mpf(case["bound"]))
        total = mp.fsum(mp.quad(f, [a, b], method="gauss-legendre") for a, b in zip(pts, pts[1:]))
        return +(2 * total * cx._mpf(case["discount"]) * mp.exp(-alpha * logK) / (2 * mp.pi))


def cm_parity(case):
    """put − call of the truncated integral: −S0 + K·D"""
    return -mp.mpf(case["S0"]) + mp.mpf(case["K"]) * mp.mpf(case["discount"])


def cm_rule_fp64(case, panels, phi):
    """hh_fourier.hip's rule under the law of phi in numpy complex128 on `panels` equal Gauss–Legendre panels"""
    v, w = fp._nodes(case["bound"], panels)
    alpha, logK = case["alpha"], math.log(case["K"])
    u = v - 1j * (alpha + 1.0)
    den = alpha * alpha + alpha - v * v + 1j * v * (2.0 * alpha + 1.0)
    kern = w * (math.exp(-alpha * logK) / (2 * math.pi) * case["discount"]) / den * np.exp(-1j * v * logK)
    return math.fsum((kern * phi(case, u)).real)


def cm_e64(case, exact_call, phi):
    """fp64 rounding of the rule on this case: its worst distance from the exact integral on 2, 4 and 8 times the
    kernel's sub-panel count (converged rules: what is left is rounding, as oracle/carr_madan_fp64.converged says)"""
    m = fp.subpanels(case["alpha"], case["bound"])
    return max(float(abs(mp.mpf(cm_rule_fp64(case, fp.PANELS * m * k, phi)) - exact_call)) for k in (2, 4, 8))


# ---- 2. the entry points, bit for bit -------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "carr_madan_pins.json")
RULES = {"m1": (1.0, 32.0), "m11": (0.5, 1000.0)}
# strikes, cps, expiries, drift rates, discount factors
BASKETS = {"one": ([105.0], [1.0], [1.0], [0.03], [0.97]),
           "three": ([90.0, 100.0, 110.0], [1.0, -1.0, 1.0], [0.5, 1.25, 0.5], [0.03, 0.02, 0.03], [0.985, 0.975, 0.985])}


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


def toolchain():
    """the compiler's own version string: a pin holds for the toolchain that built the library it was recorded on"""
    return subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.strip()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def _basket_args(name):
    arrs = [np.array(a, dtype=np.float64) for a in BASKETS[name]]
    return arrs, len(arrs[0])


def _finite(*arrays):
    assert all(np.all(np.isfinite(a)) for a in arrays)
    return sha(*arrays)


def cases():
    """-> (id, run(ctx) -> digest) of every case, in a fixed order"""
    from hedgehog_jl_amd import _ffi
    from tests import bates_cases as bt
    from tests import merton_cases as mc
    from tests import vg_cases as vc

    heston = {k: bt._FELLER_OK[k] for k in ("S0", "V0", "kappa", "theta", "sigma", "rho")}
    ln = dict(S0=mc.BASE["S0"], sigma=mc.BASE["sigma"])
    vg = next(b for b in vc.load_golden()["carr_madan"] if b["id"] == "set0")["model"]
    plain = [("lognormal", _ffi.HH_LOGNORMAL, 0, ln), ("lognormal-compat", _ffi.HH_LOGNORMAL, 1, ln),
             ("heston", _ffi.HH_HESTON, 0, heston)]

    for law, dyn, compat, params in plain:
        for rule, (alpha, bound) in RULES.items():
            for cp in (1.0, -1.0):
                def run(ctx, a=(dyn, compat, params, alpha, bound, cp)):
                    dyn, compat, params, alpha, bound, cp = a
                    m = _ffi.make_model(**params, r=0.03, T=1.25, strike=95.0, cp=cp, discount=0.965)
                    out = C.c_double()
                    ctx.check(ctx.lib.hh_carr_madan(ctx.handle, C.byref(m), dyn, compat, alpha, bound, C.byref(out)))
                    return _finite(np.array([out.value]))
                yield f"single/{law}/{rule}/cp{cp:+.0f}", run
            for basket in BASKETS:
                def run(ctx, a=(dyn, compat, params, alpha, bound, basket), grad=False):
                    dyn, compat, params, alpha, bound, basket = a
                    arrs, n = _basket_args(basket)
                    m, out, g = _ffi.make_model(**params), np.empty(n), np.empty((n, _ffi.HH_CM_GRAD_LEN))
                    args = (ctx.handle, C.byref(m), dyn, compat, alpha, bound, *[x.ctypes.data for x in arrs], n, out.ctypes.data)
                    if grad:
                        ctx.check(ctx.lib.hh_carr_madan_basket_grad(*args, g.ctypes.data))
                        return _finite(out, g)
                    ctx.check(ctx.lib.hh_carr_madan_basket(*args))
                    return _finite(out)
                yield f"basket/{law}/{rule}/{basket}", run
                yield f"grad/{law}/{rule}/{basket}", lambda ctx, run=run: run(ctx, grad=True)

    def law_call(ctx, entry, m, second, alpha, bound, basket):
        arrs, n = _basket_args(basket)
        out = np.empty(n)
        ctx.check(entry(ctx.handle, C.byref(m), C.byref(second), alpha, bound, *[x.ctypes.data for x in arrs], n, out.ctypes.data))
        return _finite(out)

    for rule, (alpha, bound) in RULES.items():
        for basket in BASKETS:
            for lam in (mc.BASE["lam"], 0.0):  # λ = 0: the compensator leaves the drift as it stands
                jump = (lam, mc.BASE["mu_j"], mc.BASE["sigma_j"])
                yield (f"jump/lam{lam:g}/{rule}/{basket}",
                       lambda ctx, a=(jump, alpha, bound, basket): law_call(ctx, ctx.lib.hh_carr_madan_jump, _ffi.make_model(**ln),
                                                                            _ffi.make_jump(*a[0]), *a[1:]))
                yield (f"bates/lam{lam:g}/{rule}/{basket}",
                       lambda ctx, a=(jump, alpha, bound, basket): law_call(ctx, ctx.lib.hh_carr_madan_bates, _ffi.make_model(**heston),
                                                                            _ffi.make_jump(*a[0]), *a[1:]))
            yield (f"vg/{rule}/{basket}",
                   lambda ctx, a=(alpha, bound, basket): law_call(ctx, ctx.lib.hh_carr_madan_vg, _ffi.make_model(S0=vg["S0"], sigma=vg["sigma"]),
                                                                  _ffi.make_vg(vg["theta"], vg["nu"]), *a))


def compute(ctx):
    """every case's digest, computed on the device through the C-ABI"""
    return {cid: run(ctx) for cid, run in cases()}
