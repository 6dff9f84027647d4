"""CPU-side checks of the batched discrete spectrum (fnft_amd_discspec_plan_* / fnft_amd_nsev_discspec_device): the
symbols are exported, and every argument check that depends on sizes, options or NULL pointers returns its code --
fnft_nsev's own code where fnft_nsev checks the same thing -- before any HIP call, so none of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest

FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_NOT_YET_IMPLEMENTED = 6

SYMBOLS = ["fnft_amd_discspec_plan_create", "fnft_amd_discspec_plan_destroy", "fnft_amd_discspec_plan_workspace_bytes",
           "fnft_amd_nsev_discspec_device", "fnft_amd_discspec_plan_finish"]
SLOW = ["BO", "CF4_2", "CF4_3", "CF5_3", "CF6_4", "ES4", "TES4"]
NEWTON = {"bound_state_localization": "NEWTON"}


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


def create_rc(capi, D, K, batch, opts=None, raw_opts=False):
    h = C.c_void_p()
    o = None if raw_opts else capi.nsev_opts(dict(NEWTON, **(opts or {})))
    rc = capi.load().fnft_amd_discspec_plan_create(C.byref(h), D, K, batch, None if o is None else C.byref(o), 0)
    assert not h, "no plan may be made from invalid arguments"
    return int(rc)


def drop_in_rc(capi, D, opts):
    """fnft_nsev on one signal with NEWTON-style arguments (it returns before touching the device here)."""
    o = capi.nsev_opts(dict(NEWTON, **(opts or {})))
    q = np.full(D, 0.5j)
    bs = np.array([1.0j, 0.5j])
    nc = np.zeros(4, np.complex128)
    rc, _ = capi.fnft_nsev(q, [-1.0, 1.0], 0, None, 1, opts=o, want_contspec=False, bound_states=bs, K=2, normconsts=nc)
    return rc


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_exported(capi, name):
    assert hasattr(capi.load(), name)
    assert name in capi.EXPORTED


# every case fails in fnft_nsev before it touches the device
DROP_IN_CASES = [(1, None), (8, {"discretization": 99}), (8, {"discretization": -1}),
                 (8, {"bound_state_localization": 7}), (8, {"bound_state_localization": -1})]
DROP_IN_CASES += [(8, {"discretization": d}) for d in SLOW]
DROP_IN_CASES += [(8, {"discretization": "CF4_2", "bound_state_localization": "FAST_EIGENVALUE"})]


@pytest.mark.parametrize("D, opts", DROP_IN_CASES)
def test_create_codes_equal_the_drop_in(capi, D, opts):
    code = drop_in_rc(capi, D, opts)
    assert code != 0
    assert create_rc(capi, D, 2, 3, opts) == code, (D, opts)


@pytest.mark.parametrize("D, K, batch, opts, code", [
    (1, 2, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 0, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 0, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discretization": 28}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_filtering": 3}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_filtering": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discspec_type": 3}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discspec_type": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_localization": "FAST_EIGENVALUE"}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 2, 1, {"bound_state_localization": "SUBSAMPLE_AND_REFINE"}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 2, 1, {"richardson_extrapolation_flag": 1}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 65536, 1, None, FNFT_EC_NOT_YET_IMPLEMENTED),              # more eigenvalues than one lane merges
    (8, 1024, 1 << 22, None, FNFT_EC_NOT_YET_IMPLEMENTED),         # more workgroups than one grid axis holds
] + [(8, 2, 1, {"discretization": d}, FNFT_EC_NOT_YET_IMPLEMENTED) for d in SLOW])
def test_create_codes(capi, D, K, batch, opts, code):
    assert create_rc(capi, D, K, batch, opts) == code


def test_null_plan_pointer_and_default_opts(capi):
    L = capi.load()
    o = capi.nsev_opts(NEWTON)
    assert L.fnft_amd_discspec_plan_create(None, 8, 2, 1, C.byref(o), 0) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_discspec_plan_create(None, 8, 2, 1, None, 0) == FNFT_EC_INVALID_ARGUMENT
    # opts == NULL: the defaults with NEWTON, so the size checks are what is left to fail
    assert create_rc(capi, 1, 2, 1, raw_opts=True) == FNFT_EC_INVALID_ARGUMENT
    assert create_rc(capi, 8, 65536, 1, raw_opts=True) == FNFT_EC_NOT_YET_IMPLEMENTED
    # the defaults themselves localize with SUBSAMPLE_AND_REFINE: passed explicitly they are refused
    d = capi.nsev_opts()
    h = C.c_void_p()
    assert L.fnft_amd_discspec_plan_create(C.byref(h), 8, 2, 1, C.byref(d), 0) == FNFT_EC_NOT_YET_IMPLEMENTED and not h


def test_call_codes_without_a_plan(capi):
    L = capi.load()
    T = (C.c_double * 2)(-1.0, 1.0)
    p = C.c_void_p(16)
    assert L.fnft_amd_nsev_discspec_device(None, p, T, p, p, p, p, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_nsev_discspec_device(None, None, None, None, None, None, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_discspec_plan_finish(None, None, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_discspec_plan_workspace_bytes(None) == 0
    L.fnft_amd_discspec_plan_destroy(None)      # ignored


def test_nsev_opts_helper(capi):
    o = capi.nsev_opts({"discretization": "4SPLIT4A", "bound_state_filtering": "BASIC", "discspec_type": "BOTH",
                        "bound_state_localization": "NEWTON", "niter": 3})
    assert (o.discretization, o.bound_state_filtering, o.discspec_type, o.bound_state_localization, o.niter) \
        == (20, 1, 2, 1, 3)
    d = capi.nsev_opts()
    assert d.niter == 10 and d.discretization == capi.NSE_DISC["2SPLIT4B"]
