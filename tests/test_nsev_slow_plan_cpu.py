"""CPU-side checks of the slow-discretization plan (fnft_amd_slow_plan_* / fnft_amd_nsev_slow_device): the symbols are
exported, every create-time argument check returns its code before any HIP call, and all seven schemes pass those checks
up to the first HIP call.  None of this needs a GPU."""
import ctypes as C

import pytest

FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_OTHER = 5

SYMBOLS = ["fnft_amd_slow_plan_create", "fnft_amd_slow_plan_destroy", "fnft_amd_slow_plan_workspace_bytes",
           "fnft_amd_nsev_slow_device", "fnft_amd_slow_plan_finish", "fnft_amd_slow_plan_chunks"]
SLOW = ["BO", "CF4_2", "CF4_3", "CF5_3", "CF6_4", "ES4", "TES4"]
FAST = ["2SPLIT2_MODAL", "2SPLIT2A", "2SPLIT4B", "2SPLIT8B", "4SPLIT4A", "4SPLIT4B"]


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


def create(capi, D, M, batch, opts=None, raw_opts=False):
    """(rc, handle) of fnft_amd_slow_plan_create; opts: dict on top of BO, raw_opts: opts == NULL."""
    h = C.c_void_p()
    o = None if raw_opts else capi.nsev_opts(dict({"discretization": "BO"}, **(opts or {})))
    rc = capi.load().fnft_amd_slow_plan_create(C.byref(h), D, M, batch, None if o is None else C.byref(o), 0)
    return int(rc), h


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_exported(capi, name):
    assert hasattr(capi.load(), name)
    assert name in capi.EXPORTED


@pytest.mark.parametrize("D, M, batch, opts, code", [
    (1, 8, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 1, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 0, 1, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 8, 0, None, FNFT_EC_INVALID_ARGUMENT),
    (8, 8, 1, {"discretization": 28}, FNFT_EC_INVALID_ARGUMENT),
    (8, 8, 1, {"discretization": -1}, FNFT_EC_INVALID_ARGUMENT),
    (8, 8, 1, {"contspec_type": 3}, -FNFT_EC_INVALID_ARGUMENT),      # wrapped twice, as fnft_nsev returns it
    (8, 8, 1, {"contspec_type": -1}, -FNFT_EC_INVALID_ARGUMENT),
    (1, 8, 1, {"contspec_type": 3}, FNFT_EC_INVALID_ARGUMENT),       # the sizes are checked first
    (8, 8, 1, {"discretization": 28, "contspec_type": 3}, FNFT_EC_INVALID_ARGUMENT),   # then the discretization
] + [(8, 8, 1, {"discretization": d}, FNFT_EC_INVALID_ARGUMENT) for d in FAST]
  + [(2, 8, 1, {"discretization": d}, FNFT_EC_INVALID_ARGUMENT) for d in SLOW[1:5]])   # the resampler wants D > 2
def test_create_codes(capi, D, M, batch, opts, code):
    rc, h = create(capi, D, M, batch, opts)
    assert rc == code
    assert not h, "no plan may be made from invalid arguments"


def test_fast_discretization_message_names_the_fast_plan(capi):
    rc, h = create(capi, 8, 8, 1, {"discretization": "2SPLIT4B"})
    assert rc == FNFT_EC_INVALID_ARGUMENT and not h
    # the text goes through the library's printf hook as ("FNFT Error: %s\n in %s(%i)...", message, function, line); a
    # hook declared with those leading arguments receives them (the variadic call passes them like fixed ones)
    seen = []
    hook_t = C.CFUNCTYPE(C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int)
    cb = hook_t(lambda fmt, msg, func, line: seen.append(msg or b"") or 0)
    L = capi.load()
    L.fnft_errwarn_setprintf(C.cast(cb, capi.PRINTF_T))
    try:
        create(capi, 8, 8, 1, {"discretization": "2SPLIT4B"})
    finally:
        capi.silence_errors()
    assert any(b"fnft_amd_plan_create" in s for s in seen), seen


def test_null_plan_pointer_and_default_opts(capi):
    L = capi.load()
    o = capi.nsev_opts({"discretization": "BO"})
    assert L.fnft_amd_slow_plan_create(None, 8, 8, 1, C.byref(o), 0) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_slow_plan_create(None, 8, 8, 1, None, 0) == FNFT_EC_INVALID_ARGUMENT
    # opts == NULL: the defaults with BO, so the size checks are what is left to fail
    assert create(capi, 1, 8, 1, raw_opts=True)[0] == FNFT_EC_INVALID_ARGUMENT


@pytest.mark.parametrize("disc", SLOW + [None])
def test_valid_arguments_reach_the_device(capi, disc):
    """Every slow scheme (None: opts == NULL) passes the checks; without a GPU the first HIP call answers
    FNFT_EC_OTHER, with one the plan exists."""
    rc, h = create(capi, 64, 16, 2, {"discretization": disc, "contspec_type": "BOTH",
                                     "richardson_extrapolation_flag": 1} if disc else None, raw_opts=disc is None)
    assert rc in (0, FNFT_EC_OTHER), rc
    assert bool(h) == (rc == 0)
    if h:
        assert capi.load().fnft_amd_slow_plan_workspace_bytes(h) > 0
        capi.load().fnft_amd_slow_plan_destroy(h)


def test_call_codes_without_a_plan(capi):
    L = capi.load()
    T = (C.c_double * 2)(-1.0, 1.0)
    p = C.c_void_p(16)
    assert L.fnft_amd_nsev_slow_device(None, p, T, p, T, 1, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_nsev_slow_device(None, None, None, None, None, 0, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_slow_plan_finish(None, None, None, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_slow_plan_workspace_bytes(None) == 0
    L.fnft_amd_slow_plan_destroy(None)      # ignored


def test_chunk_rule(capi):
    """Whole grid points per chunk, the chunks cover the signal, at least 16 grid points per chunk; few lanes -> a chunk
    for every SIMD (about two waves each), a full card -> one chunk."""
    for D, M, B in [(2, 16, 1), (31, 16, 1), (32, 16, 1), (50, 16, 1), (4096, 16, 1), (1 << 16, 16, 1), (1 << 20, 16, 3)]:
        L, nc = capi.slow_plan_chunks(D, M, B)
        assert nc * L >= D > (nc - 1) * L and (nc == 1 or L >= 16) and nc * B * ((M + 63) // 64) <= 2048
    assert capi.slow_plan_chunks(31, 16)[1] == 1 and capi.slow_plan_chunks(32, 16) == (16, 2)
    assert capi.slow_plan_chunks(50, 16) == (17, 3)
    assert capi.slow_plan_chunks(1 << 16, 16) == (32, 2048)
    assert capi.slow_plan_chunks(4096, 4096, 1)[1] > 1 and capi.slow_plan_chunks(4096, 4096, 64)[1] == 1
    assert capi.slow_plan_chunks(1, 16)[1] == 0        # no plan has these sizes
