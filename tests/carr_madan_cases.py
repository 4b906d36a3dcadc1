"""The golden Carr–Madan cases (tests/golden/carr_madan_exact.json, written by tests/golden/
make_carr_madan_exact.py) as the host and device tests read them, and the bars both hold results to."""
import json
import os

import mpmath as mp
import numpy as np

from oracle.carr_madan_fp64 import GRAD_SLOTS, grad_scales

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    """-> list of (record, case): case = the record's inputs as floats, in the form oracle/carr_madan_*.py take."""
    doc = json.load(open(os.path.join(GOLDEN_DIR, "carr_madan_exact.json")))
    assert tuple(doc["grad_slots"]) == GRAD_SLOTS
    out = []
    for r in doc["cases"]:
        c = {k: float.fromhex(v) for k, v in r["inputs"].items()}
        c.update(dynamics=r["dynamics"], cp=r["cp"], compat_sqrt_alpha=r.get("compat_sqrt_alpha", False))
        out.append((r, c))
    return out


GOLDEN = load_golden()
BY_ID = {r["id"]: (r, c) for r, c in GOLDEN}


def parity_shift(c):
    """put − call of the truncated integral, in mpmath: −S0 + K·D."""
    return -mp.mpf(c["S0"]) + mp.mpf(c["K"]) * mp.mpf(c["discount"])


def exact_price(r, c, cp):
    """The record's exact price as a call (cp = +1) or a put (−1), mpf."""
    call = mp.mpf(r["price"]) - (parity_shift(c) if c["cp"] < 0 else 0)
    return call if cp > 0 else call + parity_shift(c)


def err(got, want):
    """|float − mpf| without rounding the exact value first."""
    return float(abs(mp.mpf(float(got)) - want))


# A price may miss the exact integral by max(PRICE_FLOOR·S0, 20·e64).  e64 is fp64 rounding of the same formulas in
# numpy on a converged rule; the 20 allows for the device's exp, sincos and hypot and its summation order.  The
# floor: converged fp64 rules land within 5e-14 of the exact value at S0 = 100 (5e-16·S0) wherever nothing
# cancels, 20× that is 1e-14·S0 — 60× below the smallest miss of the plain 256-panel rule (6.2e-11 at S0 = 100, h/α = 1.56).
PRICE_FLOOR = 1e-14
# A partial may miss by max(GRAD_FLOOR·scale, 20·e64_grad), scale = max(|∂|, S0/max(|x|, 0.05)).  The converged
# fp64 restatement stays under GRAD_FLOOR/20·scale on every golden gradient (test_carr_madan_exact_host.py).
GRAD_FLOOR = 1e-11


def price_bar(r, c):
    return max(PRICE_FLOOR * c["S0"], 20.0 * float(r["e64"]))


def grad_scale(c, exact_grad):
    return grad_scales(c, [float(g) for g in exact_grad])


def grad_bar(r, c):
    exact = [mp.mpf(g) for g in r["grad"]]
    return np.maximum(GRAD_FLOOR * grad_scale(c, exact), 20.0 * np.array([float(e) for e in r["e64_grad"]]))
