"""CPU-side checks of the Richardson setters of the batched nsev plans (fnft_amd_plan_set_richardson,
fnft_amd_discspec_plan_set_richardson): the symbols are exported, a NULL plan is refused before any HIP call, and the
two create entries of the discrete-spectrum plans keep refusing the flag in opts.  No GPU needed."""
import ctypes as C

import pytest

FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_NOT_YET_IMPLEMENTED = 6

SETTERS = ["fnft_amd_plan_set_richardson", "fnft_amd_discspec_plan_set_richardson"]


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


@pytest.mark.parametrize("name", SETTERS)
def test_symbols_exported(capi, name):
    assert hasattr(capi.load(), name)
    assert name in capi.EXPORTED
    assert hasattr(capi.Plan, "set_richardson") and hasattr(capi.DiscSpecPlan, "set_richardson")
    assert capi.DiscSpecSearchPlan.set_richardson is capi.DiscSpecPlan.set_richardson


@pytest.mark.parametrize("name", SETTERS)
@pytest.mark.parametrize("enabled", (0, 1))
def test_null_plan(capi, name, enabled):
    assert getattr(capi.load(), name)(None, enabled) == FNFT_EC_INVALID_ARGUMENT


@pytest.mark.parametrize("entry,loc", [("fnft_amd_discspec_plan_create", "NEWTON"),
                                       ("fnft_amd_discspec_search_plan_create", "SUBSAMPLE_AND_REFINE"),
                                       ("fnft_amd_discspec_search_plan_create", "FAST_EIGENVALUE")])
def test_create_still_refuses_the_flag(capi, entry, loc):
    """Richardson extrapolation comes in through the setter on a created plan; the flag in opts stays refused."""
    h = C.c_void_p()
    o = capi.nsev_opts({"bound_state_localization": loc, "richardson_extrapolation_flag": 1})
    assert getattr(capi.load(), entry)(C.byref(h), 64, 2, 1, C.byref(o), 0) == FNFT_EC_NOT_YET_IMPLEMENTED
    assert not h
