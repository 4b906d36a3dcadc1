"""hedgehog.jl_amd/csrc/hh_bessel.h — the complex I_ν(z) of the Broadie–Kaya characteristic function
(the reference calls SpecialFunctions.besseli = AMOS, heston.jl:184-212) — compiled for the HOST with
g++ and checked against 40-digit mpmath on a sweep of orders and arguments covering the three
evaluation regimes (ascending series, Hankel expansion, base order + ratio recurrence), both half
planes, and the seams between them.  The same source compiles for the device; there only the
reciprocal differs (hardware rcp + two Newton steps) and a wave's lanes share the longest loop."""
import os
import shutil
import subprocess

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")
from tests.bessel_cases import cases as _cases, check_case
from tests.conftest import host_cxxflags, host_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = tmp_path / "bessel_check"
    subprocess.run(["g++", *host_cxxflags(), "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "hedgehog.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "bessel_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_besseli_against_mpmath(tmp_path):
    exe = _build(tmp_path)
    cases = _cases()
    text = "".join(f"{nu!r} {re!r} {im!r}\n" for nu, re, im in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, env=host_env()).stdout.split("\n")
    assert "table-bound-violated" not in out
    mp.mp.dps = 40
    worst = 0.0
    for (nu, re, im), line in zip(cases, out):
        lre, lim = map(float, line.split())
        err = check_case(nu, re, im, lre, lim)  # its bar: tests/bessel_cases.py
        worst = max(worst, err)
    assert worst > 0.0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_series_term_bound_holds_for_every_order(tmp_path):
    """bessel_table() finds, for its ν, a series length n0 + n1·|z| that leaves out only terms below
    2^-57 of the largest one on the whole series range, within the table size; swept over ν in (-1, 300]."""
    exe = _build(tmp_path)
    nus = np.concatenate([-1.0 + 10.0 ** np.linspace(-4, 0, 40), np.linspace(0.0, 60.0, 121), [100.0, 200.0, 300.0]])
    text = "".join(f"{float(nu)!r} 1.0 0.5\n" for nu in nus)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and "table-bound-violated" not in out.stdout
