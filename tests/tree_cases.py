"""Case table of the product-tree path tests (tests/test_tree_schedule.py, tests/test_gpu_tree_paths.py).

Each case names its entry point, sizes and form, and the kernels it must launch (names as the emulator's schedule and
the plan's launch timers print them, spaces removed).  Entries:
  fmult  fnft__poly_fmult2x2: `n` factors of degree `deg` given as exact doubles (general form), times 2^shift
  akns   fnft__akns_fscatter with an explicit r (general form from samples), akns discretization
  plan   fnft_amd_plan + transfer_matrix(b): the symmetric NSE form, `batch` signals, nse discretization
  kdv    fnft__kdv_fscatter on a real potential: the real-coefficient tree, kdv discretization
"""
import zlib

import numpy as np

import signals as S

_KDV = ["2SPLIT1A", "2SPLIT1B", "2SPLIT2A", "2SPLIT2B", "2SPLIT2S", "2SPLIT3A", "2SPLIT3B", "2SPLIT3S", "2SPLIT4A",
        "2SPLIT4B", "2SPLIT5A", "2SPLIT5B", "2SPLIT6A", "2SPLIT6B", "2SPLIT7A", "2SPLIT7B", "2SPLIT8A", "2SPLIT8B"]


def _c(id, entry, n, disc, kernels, batch=1, shift=0, signal="smooth", K=None):
    return dict(id=id, entry=entry, n=n, disc=disc, kernels=kernels, batch=batch, shift=shift, signal=signal, K=K)


def _pf(ns, ne):
    return ["KPairFft<%d,%d>" % (n, ne) for n in ns]


def _br2(ns):
    return ["KColBridge2<%d>" % n for n in ns]


# bound constants (A, B) of tests/tree_ref.err_bound, u (A log2 N + B n), one pair per form, each at most 10x the
# largest value measured on an MI355X: A from the cases with few factors, B from those with many (e / (u n))
BOUND_GENERAL = (0.06, 0.3)   # exact factors (fmult): measured 0.006 (n = 2, 3) and 0.031 (n = 300)
BOUND_SAMPLES = (2.0, 0.7)    # symmetric form and general form from samples (plan, akns): 0.36 (D = 32) and 0.068
BOUND_REAL = (2.0, 0.009)     # real-coefficient tree (kdv): 0.58 (D = 2) and 0.0012 (2SPLIT3A, D = 2^18 + 1)

P2 = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
CASES = [
    # ---- general form, exact double factors ----
    _c("fmult_d1_n2049", "fmult", 2049, 1, ["KPairSchool<1>"] + _pf(P2, 4) + ["KColFwd<4>", "KMidGen<1024>", "KColInv<4>"]),
    _c("fmult_d2_n300_up40", "fmult", 300, 2, ["KPairSchool<2>"] + _pf([16, 32, 64, 128, 256, 512], 4), shift=40),
    _c("fmult_d16_n257_dn40", "fmult", 257, 16, _pf([32, 64, 128, 256, 512, 1024, 2048], 4)
       + ["KColFwd<4>", "KColBridge2<4>", "KColInv<8>", "KMidGen<1024>"], shift=-40),
    _c("fmult_d64_n16385_bridges", "fmult", 16385, 64, _pf([128, 256, 512, 1024, 2048], 4) + ["KColFwd<4>"]
       + _br2([4, 8, 16, 32, 64, 128, 256, 512, 1024]) + ["KColInv<2048>", "KMidGen<1024>"]),
    # N > 2d on every level: degrees 3*2^j
    _c("fmult_d3_n65537_loose", "fmult", 65537, 3, ["KPairSchool<3>"] + _pf([16, 32, 64, 128, 256, 512, 1024, 2048], 4)
       + ["KColFwd<4>"] + _br2([4, 8, 16, 32, 64, 128, 256]) + ["KColInv<512>"]),
    # first split levels at longer columns (two factors of a high degree)
    _c("fmult_d4096_n2", "fmult", 2, 4096, ["KColFwd<8>", "KColInv<8>"]),
    _c("fmult_d8192_n3", "fmult", 3, 8192, ["KColFwd<16>", "KColBridge2<16>", "KColInv<32>"]),
    _c("fmult_d16384_n2", "fmult", 2, 16384, ["KColFwd<32>", "KColInv<32>"]),
    _c("fmult_d65536_n2", "fmult", 2, 65536, ["KColFwd<128>", "KColInv<128>"]),
    _c("fmult_d32768_n2", "fmult", 2, 32768, ["KColFwd<64>", "KColInv<64>"]),
    _c("fmult_d131072_n2", "fmult", 2, 131072, ["KColFwd<256>", "KColInv<256>"]),
    _c("fmult_d262144_n2", "fmult", 2, 262144, ["KColFwd<512>", "KColInv<512>"]),
    # few factors, long columns and a bridge: these kernels at the bound of (nearly) exact single products
    _c("fmult_d524288_n4", "fmult", 4, 524288, ["KColFwd<1024>", "KColBridge2<1024>", "KColInv<2048>"], K=4),
    _c("fmult_d1048576_n4", "fmult", 4, 1048576, ["KColFwd<2048>", "KColBridge2<2048>", "KColInv<4096>"], K=4),
    _c("fmult_d16_n8193", "fmult", 8193, 16, ["KColFwd<4>", "KColBridge2<128>", "KColInv<256>"]),
    _c("fmult_d32_n16385", "fmult", 16385, 32, ["KColBridge2<512>", "KColInv<1024>"]),
    # row length 2048 of the general form (N = 2^23 > 2d, product degree 2^22 + 2)
    _c("fmult_d2097153_n2_row2048", "fmult", 2, 2097153, ["KColFwd<4096>", "KMidGen<2048>", "KColInv<4096>"], K=4),
    # ---- general form from samples with an explicit r ----
    _c("akns_2SPLIT4B_D5000", "akns", 5000, "2SPLIT4B", ["KLeaf<2>", "KPairFft<16,4>", "KColFwd<4>", "KColBridge2<8>", "KColInv<16>"]),
    _c("akns_2SPLIT4A_D300", "akns", 300, "2SPLIT4A", ["KLeaf<4>", "KPairFft<16,4>", "KPairFft<2048,4>"]),
    # ---- symmetric NSE form through a plan ----
    _c("plan_MODAL_D16384", "plan", 16384, "2SPLIT2_MODAL", ["KLeafMulti<1,3>", "KMulti<128,3>", "KMulti<1024,3>",
                                                               "KMidSym<true>", "KColBridge2<4>", "KColInv<8>"]),
    _c("plan_MODAL_D32", "plan", 32, "2SPLIT2_MODAL", ["KLeafMulti<1,2>"]),
    _c("plan_MODAL_D256", "plan", 256, "2SPLIT2_MODAL", ["KLeafMulti<1,3>", "KMulti<128,2>"]),
    _c("plan_4B_D1024", "plan", 1024, "2SPLIT4B", ["KLeafMulti<2,3>", "KMulti<128,3>", "KMulti<1024,2>"]),
    _c("plan_4B_D16", "plan", 16, "2SPLIT4B", ["KLeafMulti<2,2>"]),
    _c("plan_4A_D8", "plan", 8, "2SPLIT4A", ["KLeafMulti<4,2>"]),
    _c("plan_4A_D4096", "plan", 4096, "2SPLIT4A", ["KLeafMulti<4,3>", "KMulti<128,3>", "KMulti<1024,3>"]),
    _c("plan_MODAL_D3000_pad", "plan", 3000, "2SPLIT2_MODAL", ["KLeafMulti<1,3>", "KMulti<128,3>",
                                                                 "KMulti<1024,3>"]),
    _c("plan_3A_D5000_loose", "plan", 5000, "2SPLIT3A", ["KLeaf<3>"] + _pf([16, 32, 64, 128, 256, 512, 1024, 2048, 4096], 2)
       + ["KColFwd<4>", "KColBridge2<4>", "KColBridge2<8>", "KColInv<16>"]),
    _c("plan_4B_D65536_batch3", "plan", 65536, "2SPLIT4B", ["KLeafMulti<2,3>", "KMidSym<true>", "KMidSym<false>",
                                                              "KColBridge2<4>", "KColBridge2<8>", "KColBridge2<16>",
                                                              "KColBridge2<32>", "KColInv<64>"], batch=3),
    _c("plan_MODAL_D32768_zeros", "plan", 32768, "2SPLIT2_MODAL", ["KMidSym<true>", "KColBridge2<4>", "KColInv<16>"],
       signal="zeros"),
    _c("plan_6A_D8192", "plan", 8192, "2SPLIT6A", _pf([32, 64, 128, 256, 512, 1024, 2048, 4096], 2)
       + ["KColFwd<4>", "KColBridge2<4>", "KColBridge2<8>", "KColBridge2<16>", "KColBridge2<32>", "KColInv<64>"]),
    # the largest supported tree: transform length kMaxSplitTree = 2^24, K = 4 points
    _c("plan_4A_D4194304_max", "plan", 1 << 22, "2SPLIT4A", _br2([4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
       + ["KColInv<8192>", "KMulti<1024,3>"], K=4),
    # ---- real-coefficient tree (KdV) ----
    _c("kdv_1A_D2", "kdv", 2, "2SPLIT1A", ["KRPairSchool<1>"]),
    _c("kdv_1A_D3", "kdv", 3, "2SPLIT1A", ["KRPairSchool<1>", "KRPairSchool<2>"]),
    _c("kdv_2A_D2049", "kdv", 2049, "2SPLIT2A", ["KLeaf<1>", "KRPair<8>", "KRPair<16>",
                                                    "KRPair4<32>", "KRPair4<512>", "KRPair<1024>", "KRPair<2048>"]),
    _c("kdv_2A_D262145", "kdv", 262145, "2SPLIT2A", ["KRColFwd<4>", "KRBridge<4>", "KRBridge<128>", "KRColInv<256>"]),
    _c("kdv_3A_D524289_r3", "kdv", 524289, "2SPLIT3A", ["KR3ColFwd<1>", "KR3Bridge<1>", "KR3Bridge<256>",
                                                        "KR3ColInv<512>"], K=4),
    # the last inverse column and the bridges of the real tree at every length up to the bridge limit N1 = 1024
    _c("kdv_1A_D4097", "kdv", 4097, "2SPLIT1A", ["KRColFwd<4>", "KRColInv<4>"]),
    _c("kdv_1A_D16385", "kdv", 16385, "2SPLIT1A", ["KRBridge<8>", "KRColInv<16>"]),
    _c("kdv_1A_D32769", "kdv", 32769, "2SPLIT1A", ["KRBridge<16>", "KRColInv<32>"]),
    _c("kdv_1A_D65537", "kdv", 65537, "2SPLIT1A", ["KRBridge<32>", "KRColInv<64>"]),
    _c("kdv_1A_D131073", "kdv", 131073, "2SPLIT1A", ["KRBridge<64>", "KRColInv<128>"]),
    _c("kdv_1A_D524289", "kdv", 524289, "2SPLIT1A", ["KRBridge<256>", "KRColInv<512>"], K=4),
    _c("kdv_1A_D1048577", "kdv", 1048577, "2SPLIT1A", ["KRBridge<512>", "KRColInv<1024>"], K=4),
    _c("kdv_1A_D2097153_bridge1024", "kdv", 2097153, "2SPLIT1A", ["KRBridge<1024>", "KRColInv<2048>"], K=4),
    # radix-3 columns: the last inverse column at every K
    _c("kdv_3A_D1025", "kdv", 1025, "2SPLIT3A", ["KR3ColFwd<1>", "KR3ColInv<1>"]),
    _c("kdv_3A_D2049", "kdv", 2049, "2SPLIT3A", ["KR3Bridge<1>", "KR3ColInv<2>"]),
    _c("kdv_3A_D32769", "kdv", 32769, "2SPLIT3A", ["KR3Bridge<16>", "KR3ColInv<32>"]),
    _c("kdv_3A_D65537", "kdv", 65537, "2SPLIT3A", ["KR3Bridge<32>", "KR3ColInv<64>"]),
    _c("kdv_3A_D131073", "kdv", 131073, "2SPLIT3A", ["KR3Bridge<64>", "KR3ColInv<128>"]),
    _c("kdv_3A_D262145", "kdv", 262145, "2SPLIT3A", ["KR3Bridge<128>", "KR3ColInv<256>"]),
    _c("kdv_2A_D8193", "kdv", 8193, "2SPLIT2A", ["KRColFwd<4>", "KRBridge<4>", "KRColInv<8>"]),
    _c("kdv_3A_D8193", "kdv", 8193, "2SPLIT3A", ["KLeaf<3>", "KR3ColFwd<1>", "KR3Bridge<4>", "KR3ColInv<8>"]),
    _c("kdv_6A_D4096_leaf", "kdv", 4096, "2SPLIT6A", ["KRLeafStrang<6,false>", "KR3ColInv<8>"]),
    _c("kdv_6B_D4096_leaf", "kdv", 4096, "2SPLIT6B", ["KRLeafStrang<6,true>", "KR3ColInv<4>"]),
    _c("kdv_8A_D4096_leaf", "kdv", 4096, "2SPLIT8A", ["KRLeafStrang<8,false>", "KR3Bridge<8>", "KR3ColInv<16>"]),
    _c("kdv_8B_D4096_leaf", "kdv", 4096, "2SPLIT8B", ["KRLeafStrang<8,true>"]),
]


# Kernels of the product tree: the names of the library's instantiation list (emu_kernel_list) that begin with one of
# these are the set the cases have to cover (tests/test_tree_schedule.py)
TREE_PREFIXES = ("KPair", "KMulti", "KLeaf", "KCol", "KMid", "KRPair", "KRCol", "KRBridge", "KR3", "KRLeaf")

EXCLUDED = {}
_BIG = "reachable, but only by a tree of transform length 2^24 (1 GB of coefficients per side plus the reference " \
       "work of 2^24 terms); the same template body runs at every shorter column length in the cases"
EXCLUDED.update({"KColFwd<8192>": _BIG + " (two factors of degree 2^23; KColInv<8192> runs in plan_4A_D4194304_max)"})
EXCLUDED.update({k: "reachable, but only from 2^22 + 1 real samples (4M factors): the reference work alone would take "
                 "most of the time allowed for these tests; KRColFwd<4> / KRColInv<2048> run the same bodies"
                 for k in ["KRColFwd<4096>", "KRColInv<4096>"]})


def case_ids():
    return [c["id"] for c in CASES]


def emu_args(c):
    """(entry, D, disc, batch, real) of emu_tree_schedule for a case."""
    from oracle.oracle import AKNS_DISC, NSE_DISC
    if c["entry"] == "fmult":
        return 0, c["n"], c["disc"], 1, 0
    if c["entry"] == "plan":
        return 1, c["n"], NSE_DISC[c["disc"]], c["batch"], 0
    if c["entry"] == "akns":
        return 2, c["n"], AKNS_DISC[c["disc"]], 1, 0
    return 3, c["n"], _KDV.index(c["disc"]), 1, 1


# ---- inputs ---------------------------------------------------------------------------------------------------------
def fmult_factors(c):
    """n factors of degree deg, exact doubles, times 2^shift: z^deg I plus random coefficients of total size ~0.5/sqrt(n),
    so that the product stays well conditioned like a transfer matrix (products of unstructured random factors have a
    coefficient range of hundreds of decades, and any double-precision FFT tree, the oracle's included, loses all
    digits on them)."""
    n, deg = c["n"], c["disc"]
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    sc = 0.5 / np.sqrt(2.0 * (deg + 1) * n)
    p = sc * (rng.standard_normal((4, n, deg + 1)) + 1j * rng.standard_normal((4, n, deg + 1)))
    p[0, :, 0] += 1.0
    p[3, :, 0] += 1.0
    return p.reshape(4, n * (deg + 1)) * 2.0 ** c["shift"]


def plan_signal(c, k=0):
    """(q, T) of signal k: a chirped sech pulse, shifted per signal; "zeros": pulses separated by long zero runs."""
    D = c["n"]
    T = (-20.0, 20.0)
    t = S.tgrid(T, D)
    q = (1.3 + 0.4 * k) * S.sech(t - 2.0 * k) * np.exp(1j * (0.7 + 0.3 * k) * t)
    if c["signal"] == "zeros":
        q = np.where((np.abs(t + 10.0) < 2.0) | (np.abs(t - 9.0) < 1.5), q, 0.0)
    return q.astype(np.complex128), T


def akns_signal(c):
    D = c["n"]
    T = (-10.0, 10.0)
    t = S.tgrid(T, D)
    q = (0.9 * S.sech(t) * np.exp(0.5j * t)).astype(np.complex128)
    r = (-0.6 * S.sech(t - 1.0) * np.exp(-0.2j * t)).astype(np.complex128)
    return q, r, T


def kdv_signal(c):
    D = c["n"]
    T = (-16.0, 15.0)
    return (0.8 * S.kdvv_sech(D, T)).real.astype(np.float64).astype(np.complex128), T
