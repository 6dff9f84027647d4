"""The tree -> chirp hand-over of the root (ChirpParams::root_fused: the tree's last inverse column pass done by the chirp
transform's first kernel, NftPlan::root_fusable / hand_final_to) in the CPU lane emulator, executing.  No GPU needed.

Every case runs the plan's transform twice, hand-over on and off (NftPlan::tune_fuse_root), and compares rho, a, b of
the two runs with each other and with the extended-precision reference tests/chirp_ref.py -- on the transfer matrix the
plan exports AFTER the transform, as tests/test_gpu_chirp_paths.py does -- under the bound of the NSE epilogue
(chirp_ref.err_bound with chirp_cases.BOUND_NSE).  The launches of both runs are recorded on the way: an eligible shape
shows neither KColInv nor KFinalizeScales in front of the chirp kernels and exactly one KColInv, without a second
finalize, when the matrix is exported afterwards; an ineligible shape launches what it launches with the switch off."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chirp_cases as CC
import chirp_ref as R
from oracle.oracle import NSE_DISC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_handover.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p


def _c(id, disc, D, M, batch, kappa, tree_n1, chirp_n1, eligible):
    return dict(CC._c(id, "plan", chirp_n1, disc=disc, D=D, M=M, batch=batch, kappa=kappa, cstype="BOTH"),
                tree_n1=tree_n1, eligible=eligible)


# tree_n1: column length of the tree's last split level (N = D deg0 = tree_n1 * 2048); N1: the chirp's (L = N1 * 4096)
CASES = [
    # N1 = 4: the DIRECT row kernel, a lane holds a whole column (no LDS in the column kernels)
    _c("modal_2p13_N4_batch3", "2SPLIT2_MODAL", 1 << 13, 1000, 3, 1, 4, 4, True),
    _c("4B_2p14_N16_defocusing", "2SPLIT4B", 1 << 14, 1500, 1, -1, 16, 16, True),
    # N1 = 32: the first column length that goes through LDS; M = D: L = 2N with nothing to spare
    _c("modal_2p16_N32_M_eq_D_batch2", "2SPLIT2_MODAL", 1 << 16, 1 << 16, 2, 1, 32, 32, True),
    # not eligible: L = 4N (M > D), and a padded tree (deg_tot != deg)
    _c("modal_2p13_M20000_L4N", "2SPLIT2_MODAL", 1 << 13, 20000, 1, 1, 4, 8, False),
    _c("modal_D12000_padded", "2SPLIT2_MODAL", 12000, 1000, 1, 1, 8, 4, False),
]
IDS = [c["id"] for c in CASES]


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_handover.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_arena.h", "nft_schemes.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_handover.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_handover.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                               vp, C.c_char_p, C.c_size_t]
    return L


def run(emu, c, fuse, mode=0):
    """One transform of the case: dict(out [batch, 3M], tm [batch, 4, deg+1], W [batch], names [front+tree, contspec,
    export])."""
    B, D, M = c["batch"], c["D"], c["M"]
    deg = D * CC.DEG0[c["disc"]]
    T, XI = CC.grid(c)
    q = np.concatenate(CC.nse_signals(c, T))
    out = np.zeros(B * 3 * M, np.complex128)
    tm = np.zeros(B * 4 * (deg + 1), np.complex128)
    W = np.zeros(B, np.int32)
    buf = C.create_string_buffer(1 << 16)
    Ta, Xa = np.array(T, np.float64), np.array(XI, np.float64)
    P = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    rc = emu.emu_handover(D, M, B, NSE_DISC[c["disc"]], c["kappa"], fuse, mode, P(q), P(Ta), P(Xa), P(out), P(tm), P(W),
                          buf, len(buf))
    assert rc == 0, (c["id"], rc)
    parts, cur = [], []
    for n in buf.value.decode().split("\n"):
        if n.startswith("--"):
            parts.append(cur)
            cur = []
        elif n:
            cur.append(n.replace(" ", ""))
    parts.append(cur)
    return dict(out=out.reshape(B, 3 * M), tm=tm.reshape(B, 4, deg + 1), W=W, names=parts)


@pytest.fixture(scope="module")
def runs(emu):
    """Both transforms of every case, computed once."""
    return {c["id"]: (run(emu, c, 1), run(emu, c, 0)) for c in CASES}


def _errors(c, out, other, tm, W):
    """Mass-relative errors of one signal's rho, a, b against the reference, and of the same against `other` (the run
    with the switch the other way): a and b at every point, rho -- whose metric needs H11 -- at the K points."""
    D, M = c["D"], c["M"]
    deg1 = CC.DEG0[c["disc"]]
    T, XI = CC.grid(c)
    L = CC.ROW * c["N1"]
    m = CC.out_points(c, M)
    ref = R.nsev_epilogue_ref(tm, W, T, XI, M, D, deg1, c["disc"] in ("2SPLIT2_MODAL", "2SPLIT2A"), m)
    bound = R.err_bound(CC.BOUND_NSE, L, R.phi(L, *R.nsev_grid(T, XI, M, D, deg1)) + ref["phi_pf"])
    sm = ref["mass"] * ref["scale"]
    e = dict(rho=R.quotient_error(out[m], ref["rho"], ref["H11"], ref["mass"]),
             a=R.error(out[M + m], ref["a"], sm), b=R.error(out[2 * M + m], ref["b"], sm),
             rho_ab=R.quotient_error(out[m], other[m].astype(R.CLD), ref["H11"], ref["mass"]),
             a_ab=R.error(out[M:2 * M], other[M:2 * M].astype(R.CLD), sm),
             b_ab=R.error(out[2 * M:], other[2 * M:].astype(R.CLD), sm))
    return e, bound


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_handover_values(runs, case):
    on, off = runs[case["id"]]
    for b in range(case["batch"]):
        # the matrix exported after the hand-over is the one a tree that ran its own last pass exports
        assert on["W"][b] == off["W"][b]
        assert np.array_equal(on["tm"][b], off["tm"][b])
        for name, x, y in (("on", on, off), ("off", off, on)):
            e, bound = _errors(case, x["out"][b], y["out"][b], x["tm"][b], int(x["W"][b]))
            print(case["id"], "signal", b, "hand-over", name, "bound %.3e" % bound,
                  " ".join("%s %.3e" % kv for kv in sorted(e.items())),
                  "bitwise equal" if np.array_equal(x["out"][b], y["out"][b]) else "")
            assert max(e.values()) < bound, (case["id"], b, name, e, bound)


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
