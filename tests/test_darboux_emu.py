"""The batched discrete part of the inverse transform (NftInverseDiscBatch: init, check_and_sort, run) in the CPU lane
emulator, executing the kernel bodies KInvDsPrep, KInvSolitons, KInvOp (INV_DOUBLE_Q), KBsChunk, KBsCombine, KBsPhi,
KBsPsi and KInvCdt.  No GPU needed.

Every case of tests/darboux_cases.py is held to the bound of the GPU test, FACTOR * Y(case), against the long-double
reference of tests/darboux_ref.py, and its launches are compared with the case's list.  A batch of three different
signals per (D, K) group, each against its own reference, checks the strides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import darboux_cases as DC
import darboux_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_darboux.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p
sz = C.c_size_t
U = R.U


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_darboux.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_arena.h", "nft_discspec.h", "nft_nsev_inverse.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_darboux.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_darboux.argtypes = [sz, sz, sz, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_char_p, sz]
    return L


def run(emu, cases):
    """One call for the signals `cases` of one (D, K) group: (q[B, D], launches)."""
    c0 = cases[0]
    D, K, B = c0["D"], c0["bs"].size, len(cases)
    assert all((c["D"], c["bs"].size, c["mode"], c["dstype"], c["T"]) == (D, K, c0["mode"], c0["dstype"], c0["T"])
               for c in cases)
    bs = np.ascontiguousarray(np.stack([c["bs"] for c in cases]), np.complex128)
    nc = np.ascontiguousarray(np.stack([c["nc"] for c in cases]), np.complex128)
    if c0["mode"]:
        q = np.ascontiguousarray(np.stack([DC.seed_samples(c) for c in cases]), np.complex128)
    else:
        q = np.full((B, D), np.nan + 0j)
    T = np.array(c0["T"], np.float64)
    st = np.full(B, -1, np.int32)
    names = C.create_string_buffer(1 << 14)
    rc = emu.emu_darboux(D, B, K, c0["mode"], 1 if c0["dstype"] == DC.RESIDUES else 0, bs.ctypes.data_as(vp),
                         nc.ctypes.data_as(vp), q.ctypes.data_as(vp), T.ctypes.data_as(vp), st.ctypes.data_as(vp),
                         names, len(names))
    assert rc == 0 and not st.any(), (c0["id"], rc, st)
    return q, [n.replace(" ", "") for n in names.value.decode().split("\n") if n]


def check(c, q, key=None):
    e = DC.evaluated(c)
    err = R.error(q, e["q_ref"])
    print("%s: e_emu %.1f u, e1 %.1f u, e2 %.1f u, Y %.1f u, ratio %.2f" % (key or c["id"], err / U, e["e1"] / U,
                                                                           e["e2"] / U, e["Y"] / U, err / e["Y"]))
    assert np.all(np.isfinite(q)) and err < DC.bound(c), (key or c["id"], err / U, DC.bound(c) / U)


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_ids())
def test_case_in_the_emulator(emu, case):
    assert case["D"] <= 2050
    q, names = run(emu, [case])
    check(case, q[0])
    assert names == [DC.K_PREP] + case["kernels"]


@pytest.mark.parametrize("cid", DC.BATCH_GROUPS)
def test_batch_of_three(emu, cid):
    sig = DC.batch_signals(DC.BY_ID[cid])
    q, names = run(emu, sig)
    for s, c in enumerate(sig):
        check(c, q[s], "batch[%d]%s" % (s, c["id"]))
    assert names == [DC.K_PREP] + sig[0]["kernels"]
