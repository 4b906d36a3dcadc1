"""The cases and the accuracy rule of the hh_bessel.h checks against 40-digit mpmath, shared by the host build
(tests/test_bessel_host.py) and the device build (tests/test_gpu_bessel_device.py)."""
import math

import numpy as np


def cases():
    rng = np.random.default_rng(7)
    out = []
    # ν of the parameter sets in use (H252: 0.777…; Feller-satisfied sets: 1 … 20) and the edges
    for nu in (-0.95, -0.5, -0.2, 0.0, 0.5, 7.0 / 9.0, 0.99, 1.0, 1.5, 3.0, 7.3, 15.0, 19.0, 40.0, 63.0):
        rh = max(13.0, nu * nu / 6.0 + 13.0)                  # Hankel at order ν from here (hh_bessel.h)
        radii = np.concatenate([10.0 ** rng.uniform(-2, np.log10(300.0), 36), rng.uniform(13.0, rh + 1.0, 14),
                                [12.9, 12.999, 13.0, 13.001, 13.4, 15.4, 15.6, 18.4, 18.6, 19.5,
                                 rh - 0.01, rh + 0.01, 1.5 * rh]])
        for r in radii:
            # angles on both sides of the series criterion |z| - Re z <= 14 of the in-between range
            edge = math.acos(max(-1.0, 1.0 - 14.0 / r)) if r > 7.0 else 3.0
            for ang in (0.0, 0.3, 1.2, math.pi / 2 - 1e-3, math.pi / 2 + 1e-3, 2.5, -0.7, -2.9,
                        min(edge, 1.5) - 0.01, min(edge, 1.5) + 0.01):
                out.append((float(nu), float(r * math.cos(ang)), float(r * math.sin(ang))))
    return out


def check_case(nu, re, im, lre, lim):
    """Holds log I_ν(re + i·im) = lre + i·lim (the imaginary part modulo 2π) to its bar against mpmath at the
    caller's precision; returns the relative error of I_ν."""
    import mpmath as mp
    want = mp.besseli(nu, mp.mpc(re, im))
    got = mp.exp(mp.mpc(lre, lim))
    if abs(want) > mp.mpf(10) ** 300 or abs(want) < mp.mpf(10) ** -300:
        want_l = mp.log(want)
        err = float(abs(mp.exp(mp.mpc(lre, lim) - want_l) - 1))
    else:
        err = float(abs(got - want) / abs(want))
    # The ascending series is accurate to rounding of its LARGEST terms, I_ν(|z|) in size: relative to
    # the result that is the cancellation I_ν(|z|)/|I_ν(z)|, which the dispatch keeps below e^14 (and
    # which is what the characteristic function needs: it divides by I_ν(ν_κ) >= I_ν(|ν_γ|)).  The
    # Hankel sums lose what their two exponentials cancel next to the imaginary axis (J-like zeros).
    r = math.hypot(re, im)
    near_axis = abs(abs(math.atan2(im, re)) - math.pi / 2) < 0.5
    rh = max(13.0, nu * nu / 6.0 + 13.0)
    if r < 13.0 or (nu >= 1.0 and r < rh and (r - abs(re) <= 14.0 or im * im <= 28.0 * (nu + 1.0))):
        loss = float(mp.besseli(nu, r) / abs(want)) if abs(want) > 0 else 1.0
        assert loss < 3e6 or near_axis, (nu, re, im, loss)  # e^14.9: the estimate holds away from the J-like zeros
        bar = max(2e-11, 4e-15 * loss, 1e-15 * abs(lre))
    else:
        bar = 5e-10 if near_axis else 2e-11
    assert err < bar, (nu, re, im, err)
    return err
