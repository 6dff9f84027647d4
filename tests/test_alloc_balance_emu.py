"""Every plan class allocates through one arena (fnft_amd/csrc/nft_arena.h).  Over a back end that counts
(tests/emu/emu_alloc_balance.cpp), for the smallest shapes that reach every allocation branch of the init() functions:
a successful init() followed by the end of the plan's scope leaves no block behind, and the plan's byte count is what the
back end saw requested; an init() that finds no memory at its n-th request, for every n, returns an error and leaves no
block behind either, and no block is ever handed back twice.  No kernel executes.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fnft_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_alloc_balance.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")

PLAN, SLOW, DISCSPEC, INVERSE = 0, 1, 2, 3
D = capi.NSE_DISC
CASES = {
    # NftPlan: D of the tree, M, batch, akns discretization, its degree, input samples, upsampling, kdv
    "plan-2SPLIT2_MODAL": (PLAN, [64, 16, 2, 0, 1, 64, 1, 0]),
    "plan-4SPLIT4B-resampler": (PLAN, [128, 16, 1, 10, 2, 64, 2, 0]),          # akns 4B: degree 2
    "plan-2SPLIT8B-kdv": (PLAN, [64, 16, 1, 18, 12, 64, 1, 1]),                # akns 8B: degree 12, coefficient program
    # NftSlowPlan: D, M, batch, discretization, contspec type, Richardson
    "slow-CF4_2-front-richardson": (SLOW, [64, 16, 2, D["CF4_2"], 2, 1]),      # 64 samples: the transform resampler
    "slow-BO-reduce": (SLOW, [4096, 16, 1, D["BO"], 2, 0]),                    # >= 64 chunks: the reduce stage's buffers
    # NftDiscSpecBatch: D, K, batch, discretization
    "discspec-4SPLIT4B": (DISCSPEC, [64, 3, 2, D["4SPLIT4B"]]),
    # NftInverseBatch: D, M, batch, cstype, oversampling, modal, K, discrete mode, residues
    "inverse-b-of-xi-K2": (INVERSE, [512, 512, 2, 1, 8, 1, 2, 1, 1]),          # 512 > leaf: work arrays and sub-plans
    "inverse-M0-K2": (INVERSE, [512, 0, 2, 0, 8, 1, 2, 0, 0]),
}


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_alloc_balance.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_alloc_balance.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_alloc_balance.argtypes = [C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    return L


def run(emu, kind, args, fail_at):
    a = np.array(args, np.int64)
    out = np.zeros(5, np.uint64)
    rc = emu.emu_alloc_balance(kind, a.ctypes.data_as(C.c_void_p), fail_at, out.ctypes.data_as(C.c_void_p))
    return (rc,) + tuple(int(x) for x in out)


@pytest.mark.parametrize("case", sorted(CASES))
def test_arena_balances(emu, case):
    kind, args = CASES[case]
    rc, nalloc, live, requested, class_bytes, bad = run(emu, kind, args, -1)
    print(case, "requests", nalloc, "bytes", requested)
    assert rc == 0
    assert nalloc > 0 and live == 0 and bad == 0
    assert class_bytes == requested
    for n in range(nalloc):
        rc, _, live, _, _, bad = run(emu, kind, args, n)
        assert rc != 0, (case, n)
        assert live == 0 and bad == 0, (case, n, live, bad)
