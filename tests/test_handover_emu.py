"""The tree -> chirp hand-over of the root (ChirpParams::root_fused: the tree's last inverse column pass done by the chirp
transform's first kernel, NftPlan::root_fusable / hand_final_to) in the CPU lane emulator, executing.  No GPU needed.

Every case of tests/handover_cases.py marked `emu` runs the plan's transform twice, hand-over on and off
(NftPlan::tune_fuse_root), and compares rho, a, b of the two runs with each other and with the extended-precision
reference tests/chirp_ref.py -- on the transfer matrix the plan exports AFTER the transform, as
tests/test_gpu_chirp_paths.py does -- under the bound of the NSE epilogue (chirp_ref.err_bound with
chirp_cases.BOUND_NSE).  The launches of both runs are recorded on the way: an eligible shape shows neither KColInv nor
KFinalizeScales in front of the chirp kernels and exactly one KColInv, without a second finalize, when the matrix is
exported afterwards; an ineligible shape launches what it launches with the switch off and gives the same bits.  Two
call sequences on one plan (another signal, a caller's matrix in between) run at N1 = 4 against fresh plans; the GPU
file tests/test_gpu_handover.py has them all."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chirp_cases as CC
import handover_cases as HC
from fnft_amd.capi import CSTYPE, NSE_DISC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_handover.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p

CASES = [c for c in HC.CASES if c["emu"]]
IDS = HC.ids(CASES)
SEQ = HC.case("modal_2p13_N4_batch3")   # the shape of the call sequences


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_handover.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_arena.h", "nft_schemes.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_handover.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_handover.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                               vp, C.c_int, vp, vp, vp, C.c_char_p, C.c_size_t]
    return L


def run(emu, c, fuse, mode=0, q=None, XI=None, tm_in=None, W_in=0):
    """One call of emu_handover for the case (see its modes): dict(out [outputs, batch, cs_len], tm [batch, 4, deg+1],
    W [batch], names [front+tree, contspec ..., export]).  q: the signal sets (default: set A), XI: the grids (default:
    the case's)."""
    B, D, M = c["batch"], c["D"], c["M"]
    deg = D * CC.DEG0[c["disc"]]
    T, XI0 = HC.grid(c)
    q = np.concatenate(HC.signals(c, T) if q is None else q)
    Xa = np.array(XI0 if XI is None else XI, np.float64).reshape(-1)
    nout = {2: 3, 3: 2}.get(mode, 1)
    cl = HC.CSLEN[c["cstype"]] * M
    out = np.zeros(nout * B * cl, np.complex128)
    tm = np.zeros(B * 4 * (deg + 1), np.complex128)
    W = np.zeros(B, np.int32)
    buf = C.create_string_buffer(1 << 16)
    Ta = np.array(T, np.float64)
    P = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(vp)  # noqa: E731
    rc = emu.emu_handover(D, M, B, NSE_DISC[c["disc"]], c["kappa"], CSTYPE[c["cstype"]], fuse, mode, P(q), P(Ta), P(Xa),
                          P(tm_in), W_in, P(out), P(tm), P(W), buf, len(buf))
    assert rc == 0, (c["id"], rc)
    parts, cur = [], []
    for n in buf.value.decode().split("\n"):
        if n.startswith("--"):
            parts.append(cur)
            cur = []
        elif n:
            cur.append(n.replace(" ", ""))
    parts.append(cur)
    return dict(out=out.reshape(nout, B, cl), tm=tm.reshape(B, 4, deg + 1), W=W, names=parts)


@pytest.fixture(scope="module")
def runs(emu):
    """Both transforms of every case (signal set A, the case's grid), computed once."""
    return {c["id"]: (run(emu, c, 1), run(emu, c, 0)) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_handover_values(runs, case):
    c = case
    on, off = runs[c["id"]]
    T, XI = HC.grid(c)
    m = CC.out_points(c, c["M"])
    if c["batch"] > 1:
        # the signals' roots lie in different binades: the scale KChirpRows applies differs from signal to signal
        assert len(set(on["W"].tolist())) == c["batch"] and np.any(on["W"] != 0), on["W"]
    for b in range(c["batch"]):
        # the matrix exported after the hand-over is the one a tree that ran its own last pass exports
        assert on["W"][b] == off["W"][b]
        assert np.array_equal(on["tm"][b], off["tm"][b])
        if not c["eligible"]:
            assert np.array_equal(on["out"][0, b].view(np.float64), off["out"][0, b].view(np.float64))
        ref = HC.reference(c, on["tm"][b], int(on["W"][b]), T, XI, m)
        bound = ref["bound"]
        for name, x, y in (("on", on, off), ("off", off, on)):
            e = HC.errors(c, x["out"][0, b], y["out"][0, b], ref, m)
            print(c["id"], "signal", b, "W", x["W"][b], "hand-over", name, "bound %.3e" % bound,
                  " ".join("%s %.3e" % kv for kv in sorted(e.items())),
                  "bitwise equal" if np.array_equal(x["out"][0, b], y["out"][0, b]) else "")
            assert max(e.values()) < bound, (c["id"], b, name, e, bound)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_handover_schedule(emu, runs, case):
    on, off = runs[case["id"]]
    inv = "KColInv<%d>" % case["tree_n1"]
    chirp = CC.kernels(case)
    tree0, cs0, ex0 = off["names"]
    # switch off: the tree runs its last pass, the first chirp kernel finalizes (hand_final_to), the export adds nothing
    assert tree0.count(inv) == 1 and tree0[-1] == inv and "KFinalizeScales" not in tree0 + cs0 + ex0
    assert cs0 == chirp
    assert ex0 == ["KExportTm"]
    tree1, cs1, ex1 = on["names"]
    if not case["eligible"]:
        assert (tree1, cs1, ex1) == (tree0, cs0, ex0)
    else:
        assert tree1 == tree0[:-1]                       # no KColInv (and no finalize) before the chirp kernels
        assert cs1 == cs0 and not [k for k in cs1 if k.startswith("KColInv") or k == "KFinalizeScales"]
        assert ex1 == [inv, "KExportTm"]                 # the root on demand: one KColInv, no second finalize
    # run_tree(); export_tm(): the same launches whichever way the switch is
    s1 = run(emu, case, 1, mode=1)["names"]
    s0 = run(emu, case, 0, mode=1)["names"]
    assert len(s1) == 2 and len(s0) == 2
    assert s1[0] + s1[1] == s0[0] + s0[1] == tree0 + ["KFinalizeScales", "KExportTm"]


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.float64), np.ascontiguousarray(y).view(np.float64))


@pytest.fixture(scope="module")
def fresh_b(emu):
    """Signal set B of the sequence shape on fresh plans: on the case's grid and on the other one."""
    T, XI = HC.grid(SEQ)
    sB = HC.signals(SEQ, T, "B")
    return run(emu, SEQ, 1, q=sB), run(emu, SEQ, 1, q=sB, XI=HC.other_xi(XI))


def test_another_signal_on_the_same_plan(emu, runs, fresh_b):
    """Set A, then set B on the same grids (the filter spectrum comes from the cache, v_mode 2: the column kernel's
    narrower grid), then B on another XI (a miss: the filter job's wider grid runs over chirp_col_fwd_root's early
    return) on ONE plan: each output, and the matrix exported at the end, is a fresh plan's, bit for bit -- no maximum
    (max2_out, filled by atomic max), exponent (fin_wexp, updated in place by KChirpRows) or scale survives a call."""
    c = SEQ
    T, XI = HC.grid(c)
    sA, sB = HC.signals(c, T), HC.signals(c, T, "B")
    assert not np.array_equal(runs[c["id"]][0]["W"], fresh_b[0]["W"])   # the two sets do differ in their exponents
    r = run(emu, c, 1, mode=2, q=sA + sB, XI=XI + HC.other_xi(XI))
    fresh = [runs[c["id"]][0], fresh_b[0], fresh_b[1]]
    for k in range(3):
        assert _same(r["out"][k], fresh[k]["out"][0]), k
    assert np.array_equal(r["W"], fresh[2]["W"]) and _same(r["tm"], fresh[2]["tm"])
    inv = "KColInv<%d>" % c["tree_n1"]
    tree, cs = fresh[0]["names"][:2]
    # three transforms without the tree's last pass, which runs once, for the export
    assert r["names"] == [tree, cs + tree, cs + tree, cs, [inv, "KExportTm"]], r["names"]


def test_callers_matrix_in_between(emu, runs, fresh_b):
    """A transform with the hand-over, then contspec_from_tm on another signal's matrix with W = 7, then the export: the
    from-tm output is a fresh plan's, and the exported matrix is the first signal's -- the kept scratch (root_G.Z) and
    the pending root survive a chirp run that does not consume them."""
    c = SEQ
    first = runs[c["id"]][0]
    tm_in = fresh_b[0]["tm"]
    r = run(emu, c, 1, mode=3, tm_in=tm_in, W_in=7)
    alone = run(emu, c, 1, mode=4, tm_in=tm_in, W_in=7)
    assert _same(r["out"][0], first["out"][0])
    assert _same(r["out"][1], alone["out"][0]) and np.any(alone["out"][0] != 0)
    assert np.array_equal(r["W"], first["W"]) and _same(r["tm"], first["tm"])
    inv = "KColInv<%d>" % c["tree_n1"]
    assert r["names"][2] == alone["names"][1] == CC.kernels(c) and r["names"][3] == [inv, "KExportTm"], r["names"]
