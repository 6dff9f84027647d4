"""CPU-side checks of the polynomial evaluation entries (fnft__poly_eval, fnft__poly_evalderiv,
fnft_amd_poly_eval_device, fnft_amd_nsev_eval_device): the symbols are exported and declared in the header, and the
argument checks of the two host seams return their codes -- with the reference's text through the printf hook -- before
any HIP call.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

FNFT_EC_INVALID_ARGUMENT = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fnft__poly_eval", "fnft__poly_evalderiv", "fnft_amd_poly_eval_device", "fnft_amd_nsev_eval_device"]


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_exported_and_declared(capi, name):
    assert hasattr(capi.load(), name)
    assert name in capi.EXPORTED
    with open(os.path.join(ROOT, "include", "fnft_amd.h")) as f:
        assert re.search(r"^FNFT_INT " + name + r"\(", f.read(), flags=re.M)


def test_python_wrappers_exist(capi):
    for name in ("poly_eval", "poly_evalderiv", "poly_eval_device"):
        assert callable(getattr(capi, name))
    assert callable(capi.Plan.eval_device) and capi.Plan.eval_len(None, 5, True) == 20 and capi.Plan.eval_len(None, 5) == 10


def test_host_seam_codes_and_hook_text(capi):
    """src/private/fnft__poly_eval.c:32-35, :63-66: E_INVALID_ARGUMENT(p), then (z); nz == 0 is success.  None of these
    reaches a HIP call: they return the same on a machine without a GPU."""
    L = capi.load()
    p = np.array([1.0, 2.0, 3.0], np.complex128)
    z = np.array([0.5, 2.0], np.complex128)
    d = np.zeros(2, np.complex128)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    seen = []
    hook_t = C.CFUNCTYPE(C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int)
    cb = hook_t(lambda fmt, msg, func, line: seen.append((msg, func)) or 0)
    L.fnft_errwarn_setprintf(C.cast(cb, capi.PRINTF_T))
    try:
        assert L.fnft__poly_eval(2, None, 2, P(z)) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft__poly_eval(2, P(p), 2, None) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft__poly_eval(2, None, 0, None) == FNFT_EC_INVALID_ARGUMENT      # p is checked before nz
        assert L.fnft__poly_evalderiv(2, None, 2, P(z), P(d)) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft__poly_evalderiv(2, P(p), 2, None, P(d)) == FNFT_EC_INVALID_ARGUMENT
        n = len(seen)
        assert L.fnft__poly_eval(2, P(p), 0, P(z)) == 0
        assert L.fnft__poly_evalderiv(2, P(p), 0, P(z), P(d)) == 0
        assert L.fnft__poly_evalderiv(2, P(p), 0, P(z), None) == 0                   # nothing would be written
        assert len(seen) == n
    finally:
        capi.silence_errors()
    assert seen == [(b"Invalid argument p.", b"fnft__poly_eval"), (b"Invalid argument z.", b"fnft__poly_eval"),
                    (b"Invalid argument p.", b"fnft__poly_eval"), (b"Invalid argument p.", b"fnft__poly_evalderiv"),
                    (b"Invalid argument z.", b"fnft__poly_evalderiv")], seen
    assert np.array_equal(z, [0.5, 2.0])     # untouched


def test_device_entries_argument_codes(capi):
    """The argument checks of the two device entries that need neither a device nor a plan."""
    L = capi.load()
    x = C.c_void_p(16)
    assert L.fnft_amd_poly_eval_device(3, 1, 1, None, 4, 4, 2, x, 0, x, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_poly_eval_device(3, 1, 1, x, 4, 4, 2, None, 0, x, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_poly_eval_device(3, 1, 1, x, 4, 4, 2, x, 0, None, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_poly_eval_device(3, 1, 1, x, 3, 4, 2, x, 0, x, None, None) == FNFT_EC_INVALID_ARGUMENT   # pstride
    assert L.fnft_amd_poly_eval_device(3, 1, 2, x, 4, 4, 2, x, 1, x, None, None) == FNFT_EC_INVALID_ARGUMENT   # zstride
    assert L.fnft_amd_poly_eval_device(3, 1, 1, x, 4, 4, 0, x, 0, x, None, None) == 0                          # nz == 0
    T = (C.c_double * 2)(0.0, 1.0)
    assert L.fnft_amd_nsev_eval_device(None, T, x, 4, 0, 0, x, None) == FNFT_EC_INVALID_ARGUMENT
