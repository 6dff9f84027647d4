"""CPU-side checks of the batched inverse (fnft_amd_inverse_plan_create / fnft_amd_nsev_inverse_device /
fnft_amd_inverse_plan_finish / fnft_amd_inverse_plan_destroy): the argument checks that depend on sizes and options
return fnft_nsev_inverse's codes at create time, and a NULL plan is refused -- all before any HIP call, so none of this
needs a GPU."""
import ctypes as C

import numpy as np
import pytest

FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_NOT_YET_IMPLEMENTED = 6


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


def create_rc(capi, D, M, batch, opts=None, opts_struct=None):
    h = C.c_void_p()
    o = opts_struct if opts_struct is not None else capi.inverse_opts(opts)
    rc = capi.load().fnft_amd_inverse_plan_create(C.byref(h), D, M, batch, C.byref(o), 0)
    assert not h, "no plan may be made from invalid arguments"
    return int(rc)


B_OF_XI = {"contspec_type": "B_OF_XI"}
B_OF_TAU = {"contspec_type": "B_OF_TAU"}


@pytest.mark.parametrize("D, M, batch, opts, code", [
    (6, 12, 1, None, FNFT_EC_INVALID_ARGUMENT),                         # D not a power of two
    (1, 2, 1, None, FNFT_EC_INVALID_ARGUMENT),                          # D < 2
    (8, 15, 1, None, FNFT_EC_INVALID_ARGUMENT),                         # M odd
    (8, 4, 1, None, FNFT_EC_INVALID_ARGUMENT),                          # M < D
    (8, 16, 0, None, FNFT_EC_INVALID_ARGUMENT),                         # batch 0
    (8, 16, 1, {"discretization": "2SPLIT4B"}, FNFT_EC_INVALID_ARGUMENT),
    (8, 16, 1, {"contspec_type": 7}, FNFT_EC_INVALID_ARGUMENT),         # unknown cstype
    (8, 16, 1, dict(B_OF_XI, oversampling_factor=0), -FNFT_EC_INVALID_ARGUMENT),
    (8, 16, 1, B_OF_TAU, -FNFT_EC_INVALID_ARGUMENT),                    # B_OF_TAU needs M = D
    (8, 8, 1, dict(B_OF_TAU, contspec_inversion_method="TFMATRIX_CONTAINS_REFL_COEFF"), -FNFT_EC_INVALID_ARGUMENT),
    (8, 8, 1, dict(B_OF_TAU, oversampling_factor=0), -FNFT_EC_INVALID_ARGUMENT),
])
def test_create_argument_errors_return_the_drop_in_codes(capi, D, M, batch, opts, code):
    assert create_rc(capi, D, M, batch, opts) == code


def test_create_codes_agree_with_the_drop_in(capi):
    """The same size/option errors through fnft_nsev_inverse itself (it returns before touching the device)."""
    XI = [-1.0, 1.0]
    for D, M, opts in ((6, 12, None), (8, 15, None), (8, 4, None), (8, 16, {"discretization": "2SPLIT4B"}),
                       (8, 16, {"contspec_type": 7}), (8, 16, dict(B_OF_XI, oversampling_factor=0))):
        cs = np.full(M, 0.01 + 0j)
        rc, _ = capi.fnft_nsev_inverse(M, cs, XI, None, None, D, [-1.0, 1.0], 1, opts)
        assert create_rc(capi, D, M, 1, opts) == rc, (D, M, opts)


@pytest.mark.parametrize("method", ("TFMATRIX_CONTAINS_AB_FROM_ITER", "USE_SEED_POTENTIAL_INSTEAD"))
@pytest.mark.parametrize("cstype", ("REFLECTION_COEFFICIENT", "B_OF_XI"))
def test_iteration_and_seed_methods_are_not_implemented(capi, method, cstype):
    assert create_rc(capi, 8, 16, 4, {"contspec_type": cstype, "contspec_inversion_method": method}) \
        == FNFT_EC_NOT_YET_IMPLEMENTED


def test_null_plan_is_refused(capi):
    L = capi.load()
    assert L.fnft_amd_inverse_plan_create(None, 8, 16, 1, None, 0) == FNFT_EC_INVALID_ARGUMENT
    T = (C.c_double * 2)(-1.0, 1.0)
    XI = (C.c_double * 2)(-1.0, 1.0)
    assert L.fnft_amd_nsev_inverse_device(None, C.c_void_p(16), XI, C.c_void_p(16), T, 1, None) \
        == FNFT_EC_INVALID_ARGUMENT
    st = np.zeros(4, np.int32)
    assert L.fnft_amd_inverse_plan_finish(None, None, st.ctypes.data_as(C.c_void_p), None) == FNFT_EC_INVALID_ARGUMENT
    assert (st == 0).all()
    L.fnft_amd_inverse_plan_destroy(None)   # ignored
    assert L.fnft_amd_inverse_plan_workspace_bytes(None) == 0


def test_python_wrapper_raises_with_the_code(capi):
    with pytest.raises(RuntimeError) as e:
        capi.InversePlan(8, 16, 2, {"contspec_inversion_method": "TFMATRIX_CONTAINS_AB_FROM_ITER"})
    assert e.value.rc == FNFT_EC_NOT_YET_IMPLEMENTED
