"""The Box–Muller transform of hedgehog.jl_amd/csrc/hh_rng.h ON THE DEVICE — u01_fast, two_u01_fast, neg2_log_unit,
sqrt_pos, sincospi_02, normal_pair: the GENERATE path's normals, device-only code that no host build compiles —
against long-double references on the lattices the kernels produce, at the header's claim of <= 2 ulp each.

test_device_normals_against_libm_box_muller (tests/test_gpu_parity.py) checks 2·10^6 random normals end to end to
4e-15 absolute (~18 ulp at |z| = 1); with 10^6 uniforms it never evaluates -2 ln u below u ~ 1e-6 (every normal
beyond |z| ~ 5.3) nor the seams of the quadrant reduction.  Here every binade and every seam is visited."""
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cflags():
    """The library's own compile flags (hedgehog.jl_amd/_build.py), so code generation matches the product's."""
    spec = importlib.util.spec_from_file_location("_hh_build", os.path.join(ROOT, "hedgehog.jl_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.CFLAGS)


def f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def u01(lo, hi):
    """u01_from_bits: ((w >> 12) + 1/2)·2^-52, exact in a double."""
    return (float((((hi << 32) | lo) >> 12)) + 0.5) * 2.0**-52


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("rng_device") / "rng_device_check")
    subprocess.run([hipcc, *_cflags(), "-I", os.path.join(ROOT, "hedgehog.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "rng_device_check.hip"), "-o", exe], check=True)
    text = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = {}
    for ln in text.splitlines():
        p = ln.split()
        rows.setdefault(p[0], []).append(p[1:])
    return rows


def test_fast_uniforms_are_u01_from_bits(out):
    """u01_fast builds 1.mantissa and subtracts 1 - 2^-53; two_u01_fast the same under the exponent of [2, 4):
    the uniforms of u01_from_bits (and twice them), bit for bit, on all-zero / all-one / single-bit words."""
    named = out["u01"]
    assert len(named) == 66
    for lo, hi, fast, two in named:
        lo, hi = int(lo, 16), int(hi, 16)
        want = u01(lo, hi)
        assert int(fast, 16) == b(want) and int(two, 16) == b(2.0 * want), (lo, hi)
    assert f(int(named[0][2], 16)) == 2.0**-53 and f(int(named[1][2], 16)) == 1.0 - 2.0**-53
    n, mism = out["u01_random"][0]
    assert int(n) == 10**6 and mism == "0"


def test_neg2_log_unit_on_every_binade(out):
    """-2 ln u on u = (k + 1/2)·2^-52, every binade [2^e, 2^(e+1)) of [2^-53, 1 - 2^-53]: the binade's ends, ±64 ulp
    around the sqrt(1/2) mantissa switch, 2^14 random mantissas (all of them where the binade holds fewer).  The
    reference is -2·logl(u); the header claims <= 2 ulp."""
    binades = {int(e): (int(n), float(w)) for e, n, w in out["nlog_binade"]}
    assert sorted(binades) == list(range(-53, 0))
    for e, (n, w) in binades.items():
        assert n >= min(2 ** (e + 52), 128), (e, n)   # every lattice point of the small binades, ends of the others
        assert w <= 2.0, (e, w)
    assert float(out["nlog"][0][1]) <= 2.0, out["nlog"]


def test_sqrt_pos_on_the_range_of_minus_two_log_u(out):
    n, worst, arg = out["sqrt"][0]
    assert int(n) > 10**6 and float(worst) <= 2.0, (worst, f(int(arg, 16)))


def test_sincospi_02_on_its_lattice(out):
    """sin(πt), cos(πt) for t = (k + 1/2)·2^-51 in (0, 2): ±64 lattice points around each t = j/4 (the seams of the
    quadrant reduction t = q/2 + r), within 2^-40 of 0, 1 and 2, 10^6 random t.  The reference reduces exactly in
    double and takes sinl / cosl of π_L·r: each component within 2 ulp of ITS OWN size (near a zero of one component
    that is the relative accuracy of the reduced sine), and with its quadrant's sign."""
    for name in ("sin", "cos"):
        n, worst, arg = out[name][0]
        assert int(n) > 10**6 and float(worst) <= 2.0, (name, worst, f(int(arg, 16)))
    assert out["sign_mismatch"][0] == ["0"]


# The bar of normal_pair, from the pieces' bars.  An error of k ulp of a double y is at most k·2^-52·|y|, so with
# ε = 2^-52, to first order in ε (the second-order terms are below 1e-30):
#   L = neg2_log_unit(u1)   <= 2 ulp    L(1 + δ1),   |δ1| <= 2ε
#   sqrt_pos(L)             <= 2 ulp    sqrt(-2 ln u1)·(1 + δ1/2)(1 + δ2),   |δ2| <= 2ε   (the square root halves δ1)
#   c, s of sincospi_02     <= 2 ulp    each (1 + δ3),   |δ3| <= 2ε
#   z = r·c, r·s            one rounding (1 + δ4),   |δ4| <= ε/2
# |z - z_ref| / |z_ref| <= (1 + 2 + 2 + 1/2)·ε = 5.5·2^-52, the reference being Box–Muller in long double
# (64-bit mantissa: its own error is below 2^-62 relative) from u01_from_bits of the same words.
PAIR_BAR = 5.5


def test_normal_pair_at_hand_built_words(out):
    """normal_pair on Philox blocks built by hand — u1 = 2^-53 (r = 8.57), u1 = 1 - 2^-53, binade ends and the
    sqrt(1/2) switch of u1, angles at the seams t = j/4 and at the ends of (0, 2) — and on 10^6 random blocks."""
    named = out["pairbits"]
    assert len(named) == 9 * 33
    n, worst, *words = out["pair"][0]
    assert int(n) == len(named) + 10**6
    assert float(worst) <= PAIR_BAR, (worst, words)
    # the largest normal the generator can draw: u1 = 2^-53, the angle's cosine at t = 1/2^52: r·cos to the ulp
    z = {(int(w0, 16), int(w1, 16), int(w2, 16), int(w3, 16)): (f(int(a, 16)), f(int(c, 16)))
         for w0, w1, w2, w3, a, c in named}
    z1, z2 = z[(0, 0, 0, 0)]
    r = np.sqrt(-2.0 * np.log(np.longdouble(2.0) ** -53))
    assert abs(z1 - float(r)) <= PAIR_BAR * 2.0**-52 * float(r) and 8.57 < z1 < 8.58 and 0.0 < z2 < 1e-14
