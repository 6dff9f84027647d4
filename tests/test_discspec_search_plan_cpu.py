"""CPU-side checks of the guess-free batched discrete spectrum (fnft_amd_discspec_search_plan_* /
fnft_amd_nsev_discspec_search_device / fnft_amd_discspec_plan_warnings): the symbols are exported and declared, and
every argument check that depends on sizes, options or NULL pointers returns its code before any HIP call, so none of
this needs a GPU.

Roots per signal: the degree of the transfer matrix the plan factorizes, Dsub * upsampling factor * degree per sample,
with Dsub rounded as the reference rounds it (nskip = round(D / Dsub), Dsub = round(D / nskip)) and the degree per sample
of the reference's table (2 for 2SPLIT4B, fnft__akns_discretization.c): what the drop-in uses.  For D = 1024 with the
default options that is sqrt(1024 * 100) = 320 -> nskip 3 -> Dsub 341 and 682 roots; for D = 512, 203 -> nskip 3 -> Dsub
171 and 342 roots; for (128, 2SPLIT4B, FAST_EIGENVALUE) 256 roots."""
import ctypes as C
import os
import re

import pytest

FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_NOT_YET_IMPLEMENTED = 6

SYMBOLS = ["fnft_amd_discspec_search_plan_create", "fnft_amd_discspec_search_plan_roots",
           "fnft_amd_nsev_discspec_search_device", "fnft_amd_discspec_plan_warnings"]
SLOW = ["BO", "CF4_2", "CF4_3", "CF5_3", "CF6_4", "ES4", "TES4"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


def create_rc(capi, D, K, batch, opts=None, raw_opts=False):
    h = C.c_void_p()
    o = None if raw_opts else capi.nsev_opts(opts)
    rc = capi.load().fnft_amd_discspec_search_plan_create(C.byref(h), D, K, batch, None if o is None else C.byref(o), 0)
    assert not h, "no plan may be made from invalid arguments"
    return int(rc)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_exported_and_declared(capi, name):
    assert hasattr(capi.load(), name)
    assert name in capi.EXPORTED
    with open(os.path.join(ROOT, "include", "fnft_amd.h")) as f:
        assert re.search(r"\b%s\(" % name, f.read())


@pytest.mark.parametrize("D, K, batch, opts, code", [
    (1, 2, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 0, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 0, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discretization": 28}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discretization": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_localization": 3}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_localization": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_localization": "NEWTON"}, FNFT_EC_INVALID_ARGUMENT),   # fnft_amd_discspec_plan_create
    (8, 2, 1, {"bound_state_filtering": 3}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"bound_state_filtering": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discspec_type": 3}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"discspec_type": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 2, 1, {"richardson_extrapolation_flag": 1}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 2, 1, {"richardson_extrapolation_flag": 1, "bound_state_localization": "FAST_EIGENVALUE"},
     FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 65536, 1, None, FNFT_EC_NOT_YET_IMPLEMENTED),
    # more than 16384 roots per signal: 32768 of the full signal, 4 * 8192, and 2 * 8962 of a subsampled one
    (32768, 2, 1, {"discretization": "2SPLIT2A", "bound_state_localization": "FAST_EIGENVALUE"}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8192, 2, 1, {"discretization": "2SPLIT4A", "bound_state_localization": "FAST_EIGENVALUE"}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (1 << 20, 2, 1, {"Dsub": 9000}, FNFT_EC_NOT_YET_IMPLEMENTED),
] + [(8, 2, 1, {"discretization": d}, FNFT_EC_NOT_YET_IMPLEMENTED) for d in SLOW]
  + [(8, 2, 1, {"discretization": d, "bound_state_localization": "FAST_EIGENVALUE"}, FNFT_EC_NOT_YET_IMPLEMENTED)
     for d in SLOW[:2]])
def test_create_codes(capi, D, K, batch, opts, code):
    assert create_rc(capi, D, K, batch, opts) == code


def test_null_plan_pointer_and_default_opts(capi):
    L = capi.load()
    o = capi.nsev_opts()
    assert L.fnft_amd_discspec_search_plan_create(None, 8, 2, 1, C.byref(o), 0) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_discspec_search_plan_create(None, 8, 2, 1, None, 0) == FNFT_EC_INVALID_ARGUMENT
    # opts == NULL: the defaults unchanged (SUBSAMPLE_AND_REFINE), so the size checks are what is left to fail
    assert create_rc(capi, 1, 2, 1, raw_opts=True) == FNFT_EC_INVALID_ARGUMENT
    assert create_rc(capi, 8, 0, 1, raw_opts=True) == FNFT_EC_INVALID_ARGUMENT
    assert create_rc(capi, 8, 65536, 1, raw_opts=True) == FNFT_EC_NOT_YET_IMPLEMENTED
    # NEWTON passed explicitly is the other creator's
    assert create_rc(capi, 8, 2, 1, {"bound_state_localization": "NEWTON"}) == FNFT_EC_INVALID_ARGUMENT


def test_roots(capi):
    assert capi.discspec_search_roots(1024) == (682, 341)
    assert capi.discspec_search_roots(512) == (342, 171)
    assert capi.discspec_search_roots(1024, {"Dsub": 100}) == (204, 102)
    assert capi.discspec_search_roots(128, {"discretization": "2SPLIT4B",
                                            "bound_state_localization": "FAST_EIGENVALUE"}) == (256, 128)
    assert capi.discspec_search_roots(128, {"discretization": "2SPLIT4A",
                                            "bound_state_localization": "FAST_EIGENVALUE"}) == (512, 128)
    assert capi.discspec_search_roots(256, {"discretization": "4SPLIT4B"}) == (512, 128)   # two samples per step
    assert capi.discspec_search_roots(65536) == (8192, 4096)
    assert capi.discspec_search_roots(1) == (0, 0)
    assert capi.discspec_search_roots(64, {"bound_state_localization": "NEWTON"}) == (0, 0)
    assert capi.discspec_search_roots(64, {"discretization": "BO"}) == (0, 0)
    L = capi.load()
    assert L.fnft_amd_discspec_search_plan_roots(1024, None, None) == 682       # *Dsub may be NULL


def test_call_codes_without_a_plan(capi):
    L = capi.load()
    T = (C.c_double * 2)(-1.0, 1.0)
    p = C.c_void_p(16)
    assert L.fnft_amd_nsev_discspec_search_device(None, p, T, p, p, p, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_nsev_discspec_search_device(None, None, None, None, None, None, None) == FNFT_EC_INVALID_ARGUMENT
    w = (C.c_int * 2)()
    assert L.fnft_amd_discspec_plan_warnings(None, w) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_discspec_plan_warnings(None, None) == FNFT_EC_INVALID_ARGUMENT
    # the entries both kinds of plan share
    assert L.fnft_amd_discspec_plan_finish(None, None, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_discspec_plan_workspace_bytes(None) == 0
    L.fnft_amd_discspec_plan_destroy(None)      # ignored
