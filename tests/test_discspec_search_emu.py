"""The guess-free batched discrete spectrum (nft_discspec_search.h, the body_aberthb_* and body_ds_candidates kernels
of fnft_amd/csrc/nft_kernels.h) in the CPU lane emulator against the oracle, signal by signal.  No GPU needed.

Bounds: those of the drop-in's comparison with the oracle (test_emu_kernels.py): 1e-10 absolute on the bound states
under SUBSAMPLE_AND_REFINE (both sides run Newton to the same stop), 1e-6 under FAST_EIGENVALUE (the roots of a
polynomial of degree D, no refinement); 1e-8 relative on norming constants and residues where the oracle's |a| < 1e-9."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import discspec_batch_cases as DC
from oracle.oracle import NSE_DISC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_discspec_search.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p
PAIRS = DC.PAIRS[1:4]     # (1.7, 0.4), (2.2, -0.6), (2.7, 1.0): 2, 2 and 3 bound states
BSLOC = {"FAST_EIGENVALUE": 0, "SUBSAMPLE_AND_REFINE": 2}
CASES = [("2SPLIT4B", 256, "SUBSAMPLE_AND_REFINE"), ("4SPLIT4B", 128, "SUBSAMPLE_AND_REFINE"),
         ("2SPLIT2A", 128, "FAST_EIGENVALUE")]
CHEAP = CASES[2]          # 128 roots per signal: one workgroup per signal, segment and sweep.  This case runs with
                          # several segments per sweep, the other two with one (an emulated workgroup is 256 host
                          # threads, and the fixed schedule launches every one of them)


def _P(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_discspec_search.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_discspec.h", "nft_discspec_batch.h",
                                             "nft_discspec_search.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_discspec_search.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_discspec_search.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                      C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.emu_aberthb_roots.argtypes = [C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.emu_discspec_search_lds_bytes.argtypes = [C.c_int]
    L.emu_discspec_search_lds_bytes.restype = C.c_size_t
    return L


_RUNS = {}


def run_emu(emu, disc, bsloc, q, K, niter=10, bsfilt=2, dstype=2, key=None):
    """One plan run; with a key the result is computed once and shared (never modified by the tests)."""
    if key is not None and key in _RUNS:
        return _RUNS[key]
    B, D = q.shape
    bs = np.zeros((B, K), np.complex128)
    nc = np.zeros((B, 2 * K if dstype == 2 else K), np.complex128)
    ko = np.zeros(B, np.uint64)
    st = np.zeros(B, np.int32)
    wn = np.zeros(B, np.int32)
    sz = np.zeros(3, np.uint64)
    Tn = np.array(DC.T)
    q0 = q.copy()
    rc = emu.emu_discspec_search(D, K, B, NSE_DISC[disc], BSLOC[bsloc], niter, 0, bsfilt, dstype,
                                 1 if (disc, D, bsloc) == CHEAP else 0, _P(q), _P(Tn), _P(bs), _P(nc), _P(ko), _P(st),
                                 _P(wn), _P(sz))
    assert rc == 0
    assert np.array_equal(q, q0)      # inputs are left alone
    out = (bs, nc, ko.astype(int), st, wn, sz.astype(int))
    if key is not None:
        _RUNS[key] = out
    return out


def signals(D, pairs=PAIRS):
    return np.stack([DC.signal(D, A, c) for A, c in pairs])


def oracle_ref(oracle, disc, D, bsloc, A, c):
    """(bound states, norming constants, residues, |a| at the bound states) of the oracle for one pulse."""
    q = DC.signal(D, A, c)
    rc, bs, nc, res = oracle.fnft_nsev_ds(q, DC.T, disc, bsloc=bsloc, bsfilt="FULL", niter=10)
    assert rc == 0
    four = disc.startswith("4SPLIT")
    eps_t = (DC.T[1] - DC.T[0]) / (D - 1)
    _, qp, _, _ = oracle.preprocess(q, eps_t, D, disc)
    _, a, _, _ = oracle.scatter_bound_states(qp, DC.T, bs, 2 if four else 1, skip_b=True)
    return bs, nc, res, np.abs(a)


def nearest(values, ref):
    """For every ref value the index of its nearest entry of values; asserts that the match is one to one."""
    idx = [int(np.argmin(np.abs(values - r))) for r in ref]
    assert len(set(idx)) == len(idx), (values, ref)
    return idx


@pytest.mark.parametrize("disc,D,bsloc", CASES)
def test_search_vs_oracle(emu, oracle, disc, D, bsloc):
    K = 4
    q = signals(D)
    bs, nc, ko, st, wn, sz = run_emu(emu, disc, bsloc, q, K, key=(disc, D, bsloc))
    print(disc, bsloc, "D", D, "Dsub", sz[0], "roots", sz[1], "segments", sz[2])
    assert not st.any() and not wn.any()
    bound = 1e-10 if bsloc == "SUBSAMPLE_AND_REFINE" else 1e-6
    for b, (A, c) in enumerate(PAIRS):
        bs_o, nc_o, res_o, a_o = oracle_ref(oracle, disc, D, bsloc, A, c)
        k = bs_o.size
        assert k == DC.K_OUT[1 + b]
        assert ko[b] == k, (b, ko[b], bs[b], bs_o)
        idx = nearest(bs[b, :k], bs_o)
        err = np.abs(bs[b, idx] - bs_o).max()
        print(disc, "signal", b, "K_out", k, "max |bs - oracle|", err, "oracle |a|", a_o)
        assert err < bound
        assert np.isnan(bs[b, k:]).all() and np.isnan(nc[b, k:K]).all() and np.isnan(nc[b, K + k:]).all()
        for i, j in enumerate(idx):
            if a_o[i] < 1e-9:     # b = phi/psi is independent of the grid point only at a zero of a
                assert abs(nc[b, j] - nc_o[i]) < 1e-8 * abs(nc_o[i])
                assert abs(nc[b, K + j] - res_o[i]) < 1e-8 * abs(res_o[i])


def test_zero_signal_slot(emu):
    """An all-zero signal has no bound state and status 0 (as in the oracle); the other slots do not notice it."""
    disc, D, bsloc = CHEAP
    ref = run_emu(emu, disc, bsloc, signals(D), 4, key=(disc, D, bsloc))
    q = signals(D)
    q[1] = 0.0
    bs, nc, ko, st, wn, _ = run_emu(emu, disc, bsloc, q, 4)
    assert ko[1] == 0 and st[1] == 0 and np.isnan(bs[1]).all()
    for b in (0, 2):
        assert ko[b] == ref[2][b] and st[b] == 0
        assert bs[b].tobytes() == ref[0][b].tobytes() and nc[b].tobytes() == ref[1][b].tobytes()


def test_truncation_to_K(emu):
    """K = 2 on the pulse with three bound states: two of its three, and the warning bit."""
    disc, D, bsloc = CHEAP
    ref = run_emu(emu, disc, bsloc, signals(D), 4, key=(disc, D, bsloc))
    three = ref[0][2, :3]
    bs, nc, ko, st, wn, _ = run_emu(emu, disc, bsloc, signals(D, PAIRS[2:3]), 2)
    assert ko[0] == 2 and st[0] == 0 and (wn[0] & 1)
    for v in bs[0]:
        assert np.abs(three - v).min() < 1e-9
    assert abs(bs[0, 0] - bs[0, 1]) > 0.1


def test_zero_end_coefficients(emu):
    """Polynomials with exact-zero coefficients at either end, 0 < m < n: z^nt (z^m - c) with nl leading zeros has nl
    roots at infinity, nt at zero and the m-th roots of c.  One signal keeps m >= 128 (segmented sweeps on the reduced
    degree), one drops below 128 (not segmented, like the drop-in).  The m-th roots of c are perfectly conditioned, so
    the iteration's stop (4e-14 relative) and the polish sweeps leave them at a few ulp: bound 1e-13."""
    n, c = 160, 0.5 + 0.3j
    shapes = [(10, 130, 20), (40, 96, 24)]                     # (nl, m, nt)
    tm = np.zeros((len(shapes), 4, n + 1), np.complex128)
    for b, (nl, m, nt) in enumerate(shapes):
        tm[b, 0, nl] = 1.0
        tm[b, 0, nl + m] = -c
    tm0 = tm.copy()
    z = np.zeros((len(shapes), n), np.complex128)
    mdeg = np.zeros(len(shapes), np.int32)
    st, wn, sw = (np.zeros(len(shapes), np.int32) for _ in range(3))
    sz = np.zeros(1, np.uint64)
    assert emu.emu_aberthb_roots(n, len(shapes), _P(tm), _P(z), _P(mdeg), _P(st), _P(wn), _P(sw), _P(sz)) == 0
    assert np.array_equal(tm, tm0) and not st.any() and not wn.any()
    print("sweeps", sw, "segments of the plan", sz[0])
    assert sz[0] > 1
    for b, (nl, m, nt) in enumerate(shapes):
        assert mdeg[b] == m
        assert np.isinf(z[b, m:m + nl].real).all() and (z[b, m + nl:] == 0).all()
        exact = c ** (1.0 / m) * np.exp(2j * np.pi * np.arange(m) / m)
        idx = nearest(z[b, :m], exact)
        err = np.abs(z[b, idx] - exact).max()
        print("signal", b, "m", m, "max |root - exact|", err)
        assert err < 1e-13


def test_lds_budget(emu):
    """Two workgroups of each new kernel fit the 160 KiB of a gfx950 CU."""
    for which in range(4):
        assert 2 * emu.emu_discspec_search_lds_bytes(which) <= 160 * 1024
