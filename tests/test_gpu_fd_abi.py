"""hh_fd_solve through the C-ABI: every bad argument is refused with HH_ERR_INVALID and a message, leaves the outputs
untouched, and the next valid call prices as before."""
import numpy as np
import pytest

from hedgehog_jl_amd import _ffi
from tests import fd_cases as fc

pytestmark = pytest.mark.gpu

FIELDS = ("spots", "strikes", "cps", "sigmas", "rates", "expiries", "half_widths", "styles")
SENTINEL = -12345.0


def arrays(n=3):
    S0, K, r, sigma, T = fc.CASES[0]
    a = dict(spots=np.full(n, S0), strikes=np.full(n, K), cps=np.array([-1.0, 1.0, -1.0][:n]), sigmas=np.full(n, sigma),
             rates=np.full(n, r), expiries=np.full(n, T), half_widths=np.full(n, fc.half_width(S0, K, r, sigma, T)),
             styles=np.array([1, 0, 0][:n], dtype=np.int32))
    return a


def call(ctx, M, N, R, n, a, out, **null):
    ptr = lambda k, x: None if null.get(k) else x.ctypes.data  # noqa: E731
    return ctx.lib.hh_fd_solve(ctx.handle, M, N, R, n, *(ptr(k, a[k]) for k in FIELDS), ptr("prices", out[0]),
                               ptr("deltas", out[1]), ptr("gammas", out[2]))


def fresh():
    return [np.full(3, SENTINEL) for _ in range(3)]


def test_bad_arguments_leave_the_outputs_alone_and_the_next_call_prices_as_before(hhlib):
    a = arrays()
    good = fresh()
    assert call(hhlib, 64, 10, 2, 3, a, good) == _ffi.HH_OK
    assert not any(np.any(o == SENTINEL) for o in good)

    def refused(M=64, N=10, R=2, n=3, arr=a, word=None, **null):
        out = fresh()
        assert call(hhlib, M, N, R, n, arr, out, **null) == _ffi.HH_ERR_INVALID
        msg = hhlib.lib.hh_last_error(hhlib.handle)
        assert len(msg) > 0 and (word is None or word in msg), msg
        assert all(np.all(o == SENTINEL) for o in out)
        again = fresh()
        assert call(hhlib, 64, 10, 2, 3, a, again) == _ffi.HH_OK
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, good))

    for M in (0, 2, 3, 65, -4, _ffi.HH_FD_MAX_SPACE + 2):
        refused(M=M, word=b"space_steps")
    for N in (0, -1, _ffi.HH_FD_MAX_TIME + 1):
        refused(N=N, word=b"time_steps")
    for R in (-1, 11):
        refused(R=R, word=b"rannacher_steps")
    for n in (0, (1 << 20) + 1):
        refused(n=n, word=b"options")
    for k in FIELDS + ("prices",):
        refused(word=b"NULL", **{k: True})
    bad = arrays()
    bad["styles"][1] = 2
    refused(arr=bad, word=b"style")
    # the operator condition: a drift the grid cannot carry (|b|·h/2 >= a), and a NaN anywhere in it
    bad = arrays()
    bad["rates"][2] = 40.0
    refused(arr=bad, word=b"positive")
    for field in ("sigmas", "rates", "half_widths"):
        bad = arrays()
        bad[field][0] = float("nan")
        refused(arr=bad, word=b"positive")
    bad = arrays()
    bad["half_widths"][1] = 0.0
    refused(arr=bad, word=b"positive")
