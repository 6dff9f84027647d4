"""The batched discrete-spectrum kernels (body_ds_* of fnft_amd/csrc/nft_kernels.h, host logic of
nft_discspec_batch.h) in the CPU lane emulator against the oracle, signal by signal.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import discspec_batch_cases as DC
from oracle.oracle import NSE_DISC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_discspec_batch.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p
PAIRS = DC.PAIRS[1:4]     # (1.7, 0.4), (2.2, -0.6), (2.7, 1.0): 2, 2 and 3 bound states


def _P(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_discspec_batch.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_discspec.h", "nft_discspec_batch.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_discspec_batch.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_discspec_batch.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                     vp, vp, vp, vp, vp, vp, vp]
    L.emu_discspec_lds_bytes.argtypes = [C.c_int]
    L.emu_discspec_lds_bytes.restype = C.c_size_t
    return L


def run_emu(emu, disc, q, g, niter=10, bsfilt=2, dstype=2):
    B, D = q.shape
    K = g.shape[1]
    bs = np.zeros((B, K), np.complex128)
    nc = np.zeros((B, 2 * K if dstype == 2 else K), np.complex128)
    ko = np.zeros(B, np.uint64)
    st = np.zeros(B, np.int32)
    Tn = np.array(DC.T)
    q0, g0 = q.copy(), g.copy()
    rc = emu.emu_discspec_batch(D, K, B, NSE_DISC[disc], niter, bsfilt, dstype, _P(q), _P(Tn), _P(g), _P(bs), _P(nc),
                                _P(ko), _P(st))
    assert rc == 0
    assert np.array_equal(q, q0) and np.array_equal(g, g0)      # inputs are left alone
    return bs, nc, ko.astype(int), st


# D <= kDsLdsSamples: the signal is staged in LDS; the streaming source is the same body reading global memory and is
# exercised on the GPU (test_gpu_nsev_batch_discrete.py)
@pytest.mark.parametrize("disc,D,K", [("2SPLIT4B", 300, 4), ("4SPLIT4B", 256, 3)])
def test_batch_vs_oracle(emu, oracle, disc, D, K):
    four = disc.startswith("4SPLIT")
    q, g = DC.batch(D, K, four, PAIRS)
    ref = DC.oracle_reference(oracle, disc, D, K, PAIRS)
    bs, nc, ko, st = run_emu(emu, disc, q, g)
    assert not st.any()
    for b, (rc, bs_o, nc_o, res_o, a_o) in enumerate(ref):
        assert rc == 0
        k = bs_o.size
        assert ko[b] == k, (b, ko[b], bs[b], bs_o)
        print(disc, "signal", b, "K_out", k, "max |bs - oracle|", np.abs(bs[b, :k] - bs_o).max(), "oracle |a|", a_o)
        assert np.abs(bs[b, :k] - bs_o).max() < 1e-10
        assert np.isnan(bs[b, k:]).all() and np.isnan(nc[b, k:K]).all() and np.isnan(nc[b, K + k:]).all()
        for i in range(k):
            if a_o[i] < 1e-9:     # b = phi/psi is independent of the grid point only at a zero of a
                assert abs(nc[b, i] - nc_o[i]) < 1e-8 * abs(nc_o[i])
                assert abs(nc[b, K + i] - res_o[i]) < 1e-8 * abs(res_o[i])


def test_no_filter_no_iterations(emu):
    """bsfilt NONE keeps all K slots in order; niter = 0 returns the guesses themselves."""
    q, g = DC.batch(128, 3, False, PAIRS[:2])
    bs, nc, ko, st = run_emu(emu, "2SPLIT2A", q, g, niter=0, bsfilt=0, dstype=0)
    assert (ko == 3).all() and np.array_equal(bs, g) and not st.any()
    assert np.isfinite(nc).all()


def test_lds_budget(emu):
    """Two workgroups of the LDS-resident kernels fit the 160 KiB of a gfx950 CU."""
    for which in range(4):
        assert 2 * emu.emu_discspec_lds_bytes(which) <= 160 * 1024
    assert emu.emu_discspec_lds_bytes(4) * 16 == emu.emu_discspec_lds_bytes(1) - emu.emu_discspec_lds_bytes(0)
