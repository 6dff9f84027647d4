"""CPU-side checks of the batched inverse with a discrete spectrum (fnft_amd_inverse_plan_create_discrete /
fnft_amd_nsev_inverse_discrete_device): the argument checks that depend on sizes and options return fnft_nsev_inverse's
codes at create time, and a NULL plan is refused -- all before any HIP call, so none of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest

FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_NOT_YET_IMPLEMENTED = 6
FNFT_EC_SANITY_CHECK_FAILED = 7

B_OF_XI = {"contspec_type": "B_OF_XI"}
B_OF_TAU = {"contspec_type": "B_OF_TAU"}
SEED = {"contspec_inversion_method": "USE_SEED_POTENTIAL_INSTEAD"}


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


def create_rc(capi, D, M, K, batch, opts=None):
    h = C.c_void_p()
    o = capi.inverse_opts(opts)
    rc = capi.load().fnft_amd_inverse_plan_create_discrete(C.byref(h), D, M, K, batch, C.byref(o), 0)
    assert not h, "no plan may be made from invalid arguments"
    return int(rc)


def drop_in_rc(capi, D, M, K, opts):
    """fnft_nsev_inverse on one signal with K valid bound states (it returns before touching the device here)."""
    cs = None if M == 0 else np.full(M, 0.01 + 0j)
    bs = 1j * (1.0 + np.arange(K)) if K else None
    nc = np.ones(K, np.complex128) if K else None
    rc, _ = capi.fnft_nsev_inverse(M, cs, [-1.0, 1.0], bs, nc, D, [-1.0, 1.0], 1, opts)
    return rc


# (D, M, K, opts): every case fails in fnft_nsev_inverse before it touches the device
DROP_IN_CASES = [
    (6, 12, 2, None),                                           # D not a power of two
    (6, 0, 2, None),                                            # ... without a continuous part
    (1, 0, 1, None),                                            # D < 2
    (8, 15, 2, None),                                           # M odd
    (8, 4, 2, None),                                            # M < D
    (8, 16, 2, {"discretization": "2SPLIT4B"}),
    (8, 0, 2, {"discretization": "2SPLIT4B"}),
    (8, 0, 0, None),                                            # neither contspec nor discspec
    (8, 16, 2, {"contspec_type": 7}),                           # unknown cstype
    (8, 16, 2, dict(B_OF_XI, oversampling_factor=0)),
    (8, 16, 2, B_OF_TAU),                                       # B_OF_TAU needs M = D
    (8, 8, 2, dict(B_OF_TAU, contspec_inversion_method="TFMATRIX_CONTAINS_REFL_COEFF")),
    (8, 8, 2, dict(B_OF_TAU, oversampling_factor=0)),
    (8, 16, 2, SEED),                                           # seed method with a reflection coefficient
    (8, 8, 2, dict(B_OF_TAU, **SEED)),
]


@pytest.mark.parametrize("D, M, K, opts", DROP_IN_CASES)
def test_create_codes_equal_the_drop_in(capi, D, M, K, opts):
    code = drop_in_rc(capi, D, M, K, opts)
    assert code != 0
    assert create_rc(capi, D, M, K, 3, opts) == code, (D, M, K, opts)


@pytest.mark.parametrize("D, M, K, batch, opts, code", [
    (8, 0, 2, 0, None, FNFT_EC_INVALID_ARGUMENT),                       # batch 0
    (8, 16, 0, 2, None, FNFT_EC_INVALID_ARGUMENT),                      # K = 0 with a continuous part: the K = 0 plan
    (8, 0, 0, 2, None, FNFT_EC_SANITY_CHECK_FAILED),                    # K = 0, M = 0: nothing to invert
    (8, 16, 2, 2, dict(B_OF_XI, **SEED), -FNFT_EC_INVALID_ARGUMENT),    # the drop-in refuses it after the continuous part
    (8, 16, 2, 2, {"contspec_inversion_method": "TFMATRIX_CONTAINS_AB_FROM_ITER"}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 0, 2, 2, {"contspec_inversion_method": "TFMATRIX_CONTAINS_AB_FROM_ITER"}, FNFT_EC_NOT_YET_IMPLEMENTED),
    (8, 0, 65536, 1, None, FNFT_EC_NOT_YET_IMPLEMENTED),                # more bound states than one launch holds
])
def test_create_codes_of_the_batched_call(capi, D, M, K, batch, opts, code):
    assert create_rc(capi, D, M, K, batch, opts) == code


def test_null_plan_is_refused(capi):
    L = capi.load()
    o = capi.inverse_opts()
    assert L.fnft_amd_inverse_plan_create_discrete(None, 8, 0, 2, 1, C.byref(o), 0) == FNFT_EC_INVALID_ARGUMENT
    T = (C.c_double * 2)(-1.0, 1.0)
    XI = (C.c_double * 2)(-1.0, 1.0)
    p = C.c_void_p(16)
    assert L.fnft_amd_nsev_inverse_discrete_device(None, p, XI, p, p, p, T, 1, None) == FNFT_EC_INVALID_ARGUMENT
    assert L.fnft_amd_nsev_inverse_discrete_device(None, None, None, None, None, None, None, -1, None) \
        == FNFT_EC_INVALID_ARGUMENT


@pytest.mark.parametrize("D, M, K, opts, code", [
    (8, 0, 2, {"discretization": "2SPLIT4B"}, FNFT_EC_INVALID_ARGUMENT),
    (8, 16, 2, SEED, -FNFT_EC_INVALID_ARGUMENT),
    (8, 0, 2, {"contspec_inversion_method": "TFMATRIX_CONTAINS_AB_FROM_ITER"}, FNFT_EC_NOT_YET_IMPLEMENTED),
])
def test_python_wrapper_raises_with_the_code(capi, D, M, K, opts, code):
    with pytest.raises(RuntimeError) as e:
        capi.InversePlan(D, M, 2, opts, K=K)
    assert e.value.rc == code
    assert "create_discrete" in str(e.value)
