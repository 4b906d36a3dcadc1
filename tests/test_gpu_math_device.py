"""hedgehog.jl_amd/csrc/hh_math.h on the DEVICE, the code the GPU runs: hardware reciprocal, SGPR-constant fma,
frexp / ldexp builtins, v_bitop3 sign flips — none of which the host build (tests/test_math_host.py) compiles.

- fm::sqrt_lean: the contract its header states, pinned.  The routine replaces sqrt() in cabs / csqrt of the
  Broadie–Kaya CF arithmetic (heston.jl:184-212) and drops the library routine's range scaling and class test;
  what that changes at the edges must be what the header says.
- The host test's argument sets, measure and bars (tests/c/math_cases.h, tests/math_bars.py), evaluated here.
- The device-only routines (rcp, div_by_2sqrt, sqrt_rough, exp's gradual underflow) at their stated accuracy.
- normal_quantile and atan2 bit for bit the same whichever regions share a wave."""
import os
import shutil
import struct
import subprocess

import importlib.util
import math

import pytest

from tests.math_bars import BARS, parse

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


@pytest.fixture(scope="module")
def device_out(tmp_path_factory):
    """One run of tests/c/math_device_check.hip: a handful of launches in one process."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("math_device") / "math_device_check")
    subprocess.run([hipcc, *_cflags(), "-I", os.path.join(ROOT, "hedgehog.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "math_device_check.hip"), "-o", exe], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout


def test_sqrt_lean_contract(device_out):
    out = device_out
    rows = {}
    worst = None
    for ln in out.splitlines():
        p = ln.split()
        if p[0] == "arg":
            rows[int(p[1], 16)] = (int(p[3], 16), int(p[5], 16))
        elif p[0] == "random_worst_ulp":
            worst = int(p[1])
    # the domain the callers use — zero, and everything from 2^-767 up to the largest finite double: sqrt()'s bits
    assert worst == 0
    for w in (0.0, 2.0**-767, 1.5 * 2.0**-767, 1e-200, 0.25, 1.0, 2.0, 3.0, 1e300, 1.7976931348623157e308):
        lean, ref = rows[struct.unpack("<Q", struct.pack("<d", w))[0]]
        assert lean == ref, w
    # below 2^-767 (the header: "merely less accurate, never NaN"): finite, non-negative, within 1e-3 relative
    for w in (4.9406564584124654e-324, 1e-310, 2.0**-1022, 2.0**-768):
        lean, ref = rows[struct.unpack("<Q", struct.pack("<d", w))[0]]
        assert math.isfinite(f(lean)) and f(lean) >= 0.0 and abs(f(lean) - f(ref)) <= 1e-3 * f(ref) + 1e-200, w
    # outside the contract (w finite, >= 0), stated in the header: +inf -> NaN (0 x inf), NaN -> NaN, and a negative
    # argument gives no finite positive number a caller could mistake for a modulus
    lean_inf, _ = rows[0x7FF0000000000000]
    lean_nan, _ = rows[0x7FF8000000000000]
    assert math.isnan(f(lean_inf)) and math.isnan(f(lean_nan))
    assert math.isnan(f(rows[0x8000000000000000][0]))  # -0.0: rsq = -inf passes the cap, -0 x -inf (sqrt gives -0.0)
    for neg in (-1.0, -1e-300):
        v = f(rows[struct.unpack("<Q", struct.pack("<d", neg))[0]][0])
        assert not (math.isfinite(v) and v > 0.0), (neg, v)


def test_device_build_meets_the_host_bars(device_out):
    """The host program's 2·10^6 arguments per routine (and 4·10^5 quantiles), measure and 80-bit references, with
    the special values it checks folded in the same way: the bars of tests/math_bars.py, which the host build also
    meets."""
    err = parse(device_out)
    assert set(err) == set(BARS)
    for name, bar in BARS.items():
        assert err[name][0] < bar, (name, err[name])


def test_device_only_routines_at_their_stated_accuracy(device_out):
    rows = {ln.split()[0]: ln.split() for ln in device_out.splitlines()}
    # rcp: v_rcp_f64 + two Newton steps, <= 1 ulp for normal x with normal 1/x (10^6 over the whole range + the ends)
    assert float(rows["rcp"][2]) <= 1.0, rows["rcp"]
    # div_by_2sqrt: a / (2t) from sqrt_lean's h, <= 1 ulp on the sqrt_lean domain [2^-767, 2^1000]
    assert float(rows["div2sqrt"][2]) <= 1.0, rows["div2sqrt"]
    # sqrt_rough: one v_sqrt_f64, ~2^-23 relative
    assert float(rows["sqrt_rough"][2]) <= 2.0**-23, rows["sqrt_rough"]
    # exp on [-745.2, -708] against expl: v_ldexp_f64's gradual underflow, within one denormal spacing 2^-1074
    assert float(rows["exp_under"][2]) <= 1.0, rows["exp_under"]
    # exp_finite is exp without clamp and NaN select: the same bits on the underflow range too
    assert rows["expfin_mismatch"][1] == "0"


def test_special_values(device_out):
    exp, nq, at = {}, {}, {}
    for ln in device_out.splitlines():
        p = ln.split()
        if p[:2] == ["special", "exp"]:
            exp[f(int(p[2], 16))] = (int(p[3], 16), int(p[4], 16))
        elif p[:2] == ["special", "nq"]:
            nq[f(int(p[2], 16))] = int(p[3], 16)
        elif p[:2] == ["special", "atan2"]:
            at[(int(p[2], 16), int(p[3], 16))] = int(p[4], 16)
    assert len(exp) == 6 and len(nq) == 4 and len(at) == 12
    # exp: saturation to +0 / +inf, exp(0) = 1, NaN through, and the last denormal at -745; exp_finite alike
    assert exp[-2000.0] == (0, 0) and exp[-1e6] == (0, 0) and exp[2000.0] == (b(math.inf), b(math.inf))
    assert exp[0.0][0] == b(1.0) and exp[-745.0][0] == 1
    nan_e = [v for k, v in exp.items() if math.isnan(k)][0]
    assert math.isnan(f(nan_e[0])) and math.isnan(f(nan_e[1]))
    # normal_quantile: 0 / 1 give -inf / +inf, 1/2 gives +0, NaN stays NaN
    assert nq[0.0] == b(-math.inf) and nq[1.0] == b(math.inf) and nq[0.5] == 0
    assert math.isnan(f([v for k, v in nq.items() if math.isnan(k)][0]))
    # atan2 on the axes and diagonals: the correctly rounded angles on the axes; a zero y is taken as +0 (the header:
    # the angle of the upper side, the branch besseli_logmul reflects to), so (-0, x) gives what (+0, x) gives
    pi, hpi = b(math.pi), b(math.pi / 2)
    z, nz = b(0.0), b(-0.0)
    for y in (z, nz):
        assert at[(y, b(1.0))] == z and at[(y, b(-1.0))] == pi
    for x in (z, nz):
        assert at[(b(1.0), x)] == hpi and at[(b(-1.0), x)] == b(-math.pi / 2)
    for y in (1.0, -1.0):
        for x in (1.0, -1.0):
            want = math.atan2(y, x)
            assert abs(f(at[(b(y), b(x))]) - want) <= 2.5 * math.ulp(want), (y, x)


def test_quantile_and_atan2_do_not_depend_on_the_wave(device_out):
    """normal_quantile runs its three regions (body, r <= 5 tail, far tail) as divergent branches and atan2 selects
    among three reductions and both signs: each result must be the same bits whether its wave held one region, all
    of them, or a shuffle."""
    seen = {"nq": set(), "atan2": set()}
    n = 0
    for ln in device_out.splitlines():
        p = ln.split()
        if p[0] != "div":
            continue
        seen[p[1]].add(int(p[2]))
        res = p[-3:]
        assert res[0] == res[1] == res[2], ln
        n += 1
    assert seen == {"nq": {0, 1, 2}, "atan2": {0, 1, 2}} and n == 2 * 3 * 4096
