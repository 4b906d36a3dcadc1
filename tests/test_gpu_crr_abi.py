"""hh_crr_solve through the C-ABI: every bad argument is refused with HH_ERR_INVALID and a message, and hostile
scalars (NaN, infinite, negative, huge) in every array return a status — an accepted call terminates."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, Phase, given, settings
from hypothesis import strategies as st

from hedgehog_jl_amd import _ffi

pytestmark = pytest.mark.gpu


def arrays(n, style=_ffi.HH_CRR_AMERICAN_SPOT, steps=16):
    return dict(forwards=np.full(n, 100.0), strikes=np.full(n, 100.0), cps=np.full(n, -1.0),
                ups=np.full(n, 1.02), discounts=np.full(n, 0.999), styles=np.full(n, style, dtype=np.int32),
                sf=np.full((1, steps), 0.99), rows=np.zeros(n, dtype=np.uint32))


def call(ctx, steps, n, a, n_rows=1, out=None, **null):
    out = np.empty(max(n, 1)) if out is None else out
    ptr = lambda k, x: None if null.get(k) else x.ctypes.data  # noqa: E731
    return ctx.lib.hh_crr_solve(ctx.handle, steps, n, ptr("forwards", a["forwards"]), ptr("strikes", a["strikes"]),
                                ptr("cps", a["cps"]), ptr("ups", a["ups"]), ptr("discounts", a["discounts"]),
                                ptr("styles", a["styles"]), ptr("sf", a["sf"]), n_rows, ptr("rows", a["rows"]),
                                ptr("prices", out))


def test_bad_arguments_are_refused_with_a_message(hhlib):
    a = arrays(3)
    assert call(hhlib, 16, 3, a) == _ffi.HH_OK
    for steps in (0, -1, _ffi.HH_CRR_MAX_STEPS + 1):
        assert call(hhlib, steps, 3, a) == _ffi.HH_ERR_INVALID
        assert b"steps" in hhlib.lib.hh_last_error(hhlib.handle)
    assert call(hhlib, 16, 0, a) == _ffi.HH_ERR_INVALID
    assert call(hhlib, 16, (1 << 20) + 1, a) == _ffi.HH_ERR_INVALID
    for k in ("forwards", "strikes", "cps", "ups", "discounts", "styles", "sf", "rows", "prices"):
        assert call(hhlib, 16, 3, a, **{k: True}) == _ffi.HH_ERR_INVALID, k
        assert b"NULL" in hhlib.lib.hh_last_error(hhlib.handle)
    bad = arrays(3)
    bad["styles"][1] = 3
    assert call(hhlib, 16, 3, bad) == _ffi.HH_ERR_INVALID and b"style" in hhlib.lib.hh_last_error(hhlib.handle)
    bad["styles"][1] = -1
    assert call(hhlib, 16, 3, bad) == _ffi.HH_ERR_INVALID
    bad = arrays(3)
    bad["rows"][2] = 1
    assert call(hhlib, 16, 3, bad) == _ffi.HH_ERR_INVALID and b"row" in hhlib.lib.hh_last_error(hhlib.handle)
    assert call(hhlib, 16, 3, arrays(3), n_rows=0) == _ffi.HH_ERR_INVALID
    assert call(hhlib, 16, 3, arrays(3), n_rows=4) == _ffi.HH_ERR_INVALID
    # no Spot American tree: the spot-factor arguments are not read
    eu = arrays(3, style=_ffi.HH_CRR_EUROPEAN)
    assert call(hhlib, 16, 3, eu, n_rows=0, sf=True, rows=True) == _ffi.HH_OK


weird = st.one_of(st.floats(allow_nan=True, allow_infinity=True, width=64),
                  st.sampled_from([0.0, -0.0, 1e-320, 1e-300, 1e300, -1.0, 1.0, 2.0, 100.0, float("nan"),
                                   float("inf"), -float("inf")]))


@settings(max_examples=int(os.environ.get("HH_FUZZ_EXAMPLES", "300")), deadline=None, derandomize=True, database=None,
          phases=[Phase.explicit, Phase.generate], suppress_health_check=[HealthCheck.function_scoped_fixture,
                                                                            HealthCheck.too_slow])
@given(field=st.sampled_from(["forwards", "strikes", "cps", "ups", "discounts", "sf"]), vals=st.lists(weird, min_size=3,
       max_size=3), steps=st.sampled_from([-5, 0, 1, 7, 64, 65, 300, 2048, 2049, _ffi.HH_CRR_MAX_STEPS + 1]),
       style=st.sampled_from([0, 1, 2, 2, 3, -7]), row=st.sampled_from([0, 0, 1, 2**31]),
       n_rows=st.sampled_from([0, 1, 1, 2, 5]))
def test_hostile_scalars_return_a_status(hhlib, field, vals, steps, style, row, n_rows):
    n = 3
    a = arrays(n, steps=max(steps, 1) if 0 < steps <= _ffi.HH_CRR_MAX_STEPS else 1)
    a["sf"] = np.full((max(n_rows, 1), a["sf"].shape[1]), 0.99)
    a["styles"][0] = style
    a["rows"][1] = row
    if field == "sf":
        a["sf"].flat[:3] = vals[:min(3, a["sf"].size)]
    else:
        a[field][:] = vals
    out = np.full(n, -12345.0)
    rc = call(hhlib, steps, n, a, n_rows=n_rows, out=out)
    assert rc in (_ffi.HH_OK, _ffi.HH_ERR_INVALID), rc
    if rc != _ffi.HH_OK:
        assert len(hhlib.lib.hh_last_error(hhlib.handle)) > 0
    else:
        assert not np.any(out == -12345.0)   # every tree wrote its price (possibly NaN)
