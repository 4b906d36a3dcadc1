"""hedgehog.jl_amd/csrc/hh_bessel.h ON THE DEVICE, in the waves the Broadie–Kaya kernels run it in.

The Horner loops of besseli_series / besseli_asym run to the longest count among a wave's active lanes
(wave_max6 + readfirstlane) and per-lane guards (m <= Mh, m <= M) skip the steps a lane does not need, so by
construction a lane's result must not depend on which lanes share its wave or how many are active.  The host build
(tests/test_bessel_host.py) cannot see that: there wave_max6 returns the lane's own count.  Here the host test's
cases (tests/bessel_cases.py) run, one order per launch with the tables read through a device pointer as
bk_cf_kernel reads them, in four lane layouts (tests/c/bessel_device_check.hip): isolated (lane 0 alone in its
wave), sweep order, a seeded shuffle, and adversarial waves that put every case beside the order's longest series
sum, longest Hankel sum and a recurrence-branch case."""
import importlib.util
import math
import os
import shutil
import struct
import subprocess

import mpmath as mp
import pytest

from tests.bessel_cases import cases, check_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_flags():
    """The library's compile flags and hh_bk.hip's own unit flags (hedgehog.jl_amd/_build.py): the code
    generation of the Broadie–Kaya unit, which inlines these functions."""
    spec = importlib.util.spec_from_file_location("_hh_build", os.path.join(ROOT, "hedgehog.jl_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    unit = [flags for src, _, flags in mod.UNITS if src == "hh_bk.hip"][0]
    assert "-disable-machine-licm" in unit
    return list(mod.CFLAGS) + list(unit)


def f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("bessel_device") / "bessel_device_check")
    subprocess.run([hipcc, *_build_flags(), "-I", os.path.join(ROOT, "hedgehog.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "bessel_device_check.hip"), "-o", exe], check=True)
    cs = cases()
    text = "".join(f"{nu!r} {re!r} {im!r}\n" for nu, re, im in cs)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    return cs, p


def _iso(run):
    cs, p = run
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [ln.split()[1:] for ln in p.stdout.splitlines() if ln.startswith("iso ")]
    assert len(rows) == len(cs) == 9450
    for (nu, re, im), r in zip(cs, rows):
        assert (float(r[0]), float(r[1]), float(r[2])) == (nu, re, im)
    return cs, [[int(x, 16) for x in r[3:]] for r in rows]


def test_tables_meet_their_bound(run):
    """(d) bessel_table() finds a series length for every order of the cases (and for ν − n_int)."""
    cs, p = run
    assert "table-bound-violated" not in p.stdout
    assert p.returncode == 0, p.stderr[-2000:]


def test_result_does_not_depend_on_the_wave(run):
    """(a) Every active lane of the sweep, shuffled and adversarial layouts — each case beside the longest series
    sum, the longest Hankel sum and (orders >= 1) a recurrence case, waves mixing the three, ragged last waves —
    gives the bits of the same case alone in its wave: (lg, mul), and besseli_logmul_re on the real axis."""
    cs, p = run
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [list(map(int, ln.split()[1:])) for ln in p.stdout.splitlines() if ln.startswith("layout ")]
    n_orders = len({nu for nu, _, _ in cs})
    assert len(rows) == 3 * n_orders
    for nu_index, layout, active, bad, n_comp in rows:
        assert bad == 0, (nu_index, layout, bad, [ln for ln in p.stdout.splitlines() if ln.startswith("first-")])
        assert active >= 630 if layout < 3 else active >= 630 * (n_comp + 1) * 64
    # the adversarial waves held all three regimes wherever the cases reach the recurrence: orders >= 1 whose
    # R_h = ν²/6 + 13 exceeds 14 (below that, |z| - Re z <= |z| < 14 sends the whole in-between range to the series)
    comps = {nu_index: n_comp for nu_index, layout, _, _, n_comp in rows}
    orders = list(dict.fromkeys(nu for nu, _, _ in cs))
    assert [comps[i] for i in range(len(orders))] == [3 if nu >= 1.0 and nu * nu / 6.0 + 13.0 > 14.0 else 2
                                                      for nu in orders]


def test_isolated_lanes_against_mpmath(run):
    """(b) The isolated layout against 40-digit mpmath.besseli, at the host test's bars."""
    cs, iso = _iso(run)
    mp.mp.dps = 40
    worst = 0.0
    for (nu, re, im), (lg_re, lg_im, mul_re, mul_im, *_) in zip(cs, iso):
        mr, mi = f(mul_re), f(mul_im)
        lre = f(lg_re) + math.log(math.hypot(mr, mi))
        lim = f(lg_im) + math.atan2(mi, mr)
        worst = max(worst, check_case(nu, re, im, lre, lim))
    assert worst > 0.0


def test_real_axis_form_is_the_complex_real_parts(run):
    """(c) On the positive real axis besseli_logmul_re returns the complex form's real parts, bit for bit."""
    cs, iso = _iso(run)
    n = 0
    for (nu, re, im), r in zip(cs, iso):
        if im == 0.0 and re > 0.0:
            assert len(r) == 6 and r[4] == r[0] and r[5] == r[2], (nu, re)
            n += 1
    assert n == 15 * 63
