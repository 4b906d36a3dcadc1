"""The accuracy bars of hedgehog.jl_amd/csrc/hh_math.h, in ulp of the fp64 result, over the argument sets of
tests/c/math_cases.h: one place for the host build (tests/test_math_host.py) and the device build
(tests/test_gpu_math_device.py), which are held to the same numbers.  Each error must be strictly below its bar."""

BARS = {
    "sin": 2.0, "cos": 2.0,        # (absolute 2^-73 where the value is below 1e-6)
    "log": 2.5, "atan2": 2.5,
    "exp": 1.5,
    "wsin": 2.0, "wcos": 2.0,      # the wide sincos (|x| <= 2^45, three-term reduction) as good as the narrow one
    "nquant": 8.0,                 # AS 241: a rational approximation good to 1e-16 before rounding; it seeds a root search
}


def parse(out):
    """{name: (error, [argument bits])} from the programs' "name samples error arg [arg2]" lines."""
    err = {}
    for ln in out.strip().splitlines():
        p = ln.split()
        if p[0] in BARS:
            err[p[0]] = (float(p[2]), [int(b, 16) for b in p[3:]])
    return err
