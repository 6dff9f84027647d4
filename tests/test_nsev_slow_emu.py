"""The slow-discretization kernels (body_slow_* of fnft_amd/csrc/nft_kernels.h) and the plan's host logic
(nft_nsev_slow.h) in the CPU lane emulator against the extended-precision restatement tests/slow_ref.py: all seven
schemes, kappa = +1 and -1, one small shape each, a multi-chunk shape and a Richardson pass.  Bound as on the GPU
(tests/test_gpu_nsev_slow.py): max |X - X_ld| / max |X_ld| <= 4 e_dbl for rho, a and b, e_dbl being the same figure of the
restatement run in double.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import slow_cases as SC
from fnft_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_nsev_slow.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p


def _P(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_nsev_slow.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_discspec.h", "nft_nsev_slow.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_nsev_slow.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_nsev_slow.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int,
                                vp, vp, vp]
    return L


def run_emu(emu, disc, q, T, M, kappa, cstype=2, richardson=0):
    B, D = q.shape
    out = np.zeros((B, M * capi.CS_FACTOR[cstype]), np.complex128)
    st = np.zeros(B, np.int32)
    wn = np.zeros(B, np.int32)
    q0 = q.copy()
    rc = emu.emu_nsev_slow(D, M, B, capi.NSE_DISC[disc], cstype, richardson, _P(q), _P(np.array(T, np.float64)),
                           _P(np.array(SC.XI, np.float64)), kappa, _P(out), _P(st), _P(wn))
    assert rc == 0
    assert np.array_equal(q, q0)            # the input is left alone
    return out, st, wn


@pytest.mark.parametrize("kappa", [1, -1])
@pytest.mark.parametrize("disc", SC.DISCS)
def test_small_shape(emu, disc, kappa):
    D, M = 24, 5
    q = SC.signal(D, kappa)[None, :].copy()
    out, st, wn = run_emu(emu, disc, q, SC.interval(kappa), M, kappa)
    assert not st.any()
    SC.check("emu", SC.split_both(out[0], M), disc, kappa, D, M)


@pytest.mark.parametrize("D", [39, 40])
@pytest.mark.parametrize("disc", ["CF4_2", "CF6_4"])
def test_resampler_threshold(emu, disc, D):
    """The last size whose shifted copies are summed directly and the first that goes through the transform resampler."""
    M = 16
    q = SC.signal(D, 1)[None, :].copy()
    out, st, wn = run_emu(emu, disc, q, SC.interval(1), M, 1)
    assert not st.any()
    SC.check("emu", SC.split_both(out[0], M), disc, 1, D, M)


@pytest.mark.parametrize("disc,richardson", [("CF5_3", 0), ("ES4", 0), ("TES4", 1), ("CF4_2", 1)])
def test_multi_chunk(emu, disc, richardson):
    """Three chunks with a ragged last one (the full pass), two signals; with Richardson the second pass has two."""
    D, M, B = 50, 5, 2
    L, nc = capi.slow_plan_chunks(D, M, B)
    assert nc == 3 and D % L != 0
    q = np.stack([SC.signal(D, 1, v) for v in range(B)])
    out, st, wn = run_emu(emu, disc, q, SC.interval(1), M, 1, richardson=richardson)
    assert not st.any()
    for b in range(B):
        SC.check("emu", SC.split_both(out[b], M), disc, 1, D, M, richardson, variant=b)


@pytest.mark.parametrize("disc,richardson", [("BO", 0), ("ES4", 1)])
def test_reduce_stage(emu, disc, richardson):
    """65 chunks of 17 grid points with a ragged last one: from 64 chunks on the maps are multiplied in groups first
    (9 per group, the last group ragged too); the Richardson pass has 33 chunks in 4 groups."""
    D, M = 1100, 5
    assert capi.slow_plan_chunks(D, M, 1) == (17, 65)
    q = SC.signal(D, 1)[None, :].copy()
    out, st, wn = run_emu(emu, disc, q, SC.interval(1), M, 1, richardson=richardson)
    assert not st.any()
    SC.check("emu", SC.split_both(out[0], M), disc, 1, D, M, richardson)


def test_status_bit_where_a_is_exactly_zero(emu):
    """a(xi) = 0 exactly sets the signal's status bit and nobody else's.  Two real samples A, B under BO at xi = 0 give
    S11 = cos(A e) cos(B e) - sin(A e) sin(B e) as a difference of two rounded products, which is exactly 0 for some B
    within a few ulps of pi/2 - A; the emulator's arithmetic is the host's libm, so the test searches those neighbours
    (one call, 246 signals) instead of naming one.  The GPU file has no such case: the device's sincos decides there."""
    T, XI, M = np.array([0.0, 1.0]), np.array([-1.0, 1.0]), 3      # eps_t = 1; xi = 0 is the middle grid point
    sig = []
    for A in np.linspace(0.5, 0.7, 6):
        lo = hi = np.pi / 2 - A
        sig.append((A, lo))
        for _ in range(20):
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 2.0)
            sig += [(A, lo), (A, hi)]
    q = np.array(sig, np.complex128)
    B = q.shape[0]
    out = np.zeros((B, 3 * M), np.complex128)
    st = np.zeros(B, np.int32)
    wn = np.zeros(B, np.int32)
    assert emu.emu_nsev_slow(2, M, B, capi.NSE_DISC["BO"], 2, 0, _P(q), _P(T), _P(XI), 1, _P(out), _P(st), _P(wn)) == 0
    a_mid = out[:, M + 1]
    assert st.any(), "no exact zero among the neighbours"
    assert np.array_equal(st != 0, a_mid == 0)                     # the bit is set exactly where a == 0
    ok = np.nonzero(st == 0)[0]
    assert np.isfinite(out[ok]).all()
    b = int(ok[0])                                                 # a slot next to failing ones: same as on its own
    alone = np.zeros((1, 3 * M), np.complex128)
    s1, w1 = np.zeros(1, np.int32), np.zeros(1, np.int32)
    qb = q[b:b + 1].copy()
    assert emu.emu_nsev_slow(2, M, 1, capi.NSE_DISC["BO"], 2, 0, _P(qb), _P(T), _P(XI), 1, _P(alone), _P(s1), _P(w1)) == 0
    assert np.array_equal(alone[0], out[b]) and not s1.any()


def test_contspec_types_agree(emu):
    D, M = 24, 5
    q = SC.signal(D, 1)[None, :].copy()
    both, _, _ = run_emu(emu, "CF4_3", q, SC.interval(1), M, 1, cstype=2)
    rho, _, _ = run_emu(emu, "CF4_3", q, SC.interval(1), M, 1, cstype=0)
    ab, _, _ = run_emu(emu, "CF4_3", q, SC.interval(1), M, 1, cstype=1)
    assert np.array_equal(rho[0], both[0, :M]) and np.array_equal(ab[0], both[0, M:])
