"""Case table of the chirp z-transform path tests (tests/test_chirp_schedule.py, tests/test_gpu_chirp_paths.py).

The chirp transform of length L = 4096 N1 runs three launches (run_chirp, nft_chirp.h): KChirpColFwd<N1, DFT>, KChirpRows,
KChirpColInv<N1, DFT, KDV>.  Each case names its entry point, sizes and mode, and the column length N1 it must reach;
the kernels it must launch follow from those (names as the emulator's schedule and the plans' launch timers print them,
spaces removed).  Entries:
  chirpz    fnft__poly_chirpz (raw values, cstype -1): a polynomial of degree `deg`, M outputs
  resample  fnft__misc_resample (DFT mode: npoly 1 forward, then npoly 2 inverse), D samples
  plan      fnft_amd_plan + contspec_device: the NSE epilogue on the plan's own tree, `batch` signals
  cache     one plan called again with another signal on the same grid (filter spectrum reloaded, v_mode 2)
  tm        contspec_from_tm_device: the NSE epilogue on caller transfer matrices (poly_tm), exponent W != 0
  kdv       fnft_amd_kdvv_plan + contspec_device: the KdV epilogue, real-coefficient (real=1) or complex tree
Grids: "tight" chooses the chirp points so that the largest chirp phase Phi (tests/chirp_ref.phi) stays near log2 L --
the kernels' own accuracy is then what the bound pins -- with xi of order one; "wide" is a realistic fnft_nsev /
root-finder grid whose Phi term dominates.
"""
import zlib

import numpy as np

ROW = 4096   # kRowChirp: N2 of the chirp's split transforms


def _c(id, entry, N1, **kw):
    d = dict(id=id, entry=entry, N1=N1, K=None, absent=[], grid="tight", batch=1)
    d.update(kw)
    return d


def kernels(c):
    """The chirp kernels a case must launch."""
    n1 = c["N1"]
    if c["entry"] == "resample":
        return ["KChirpColFwd<%d,true>" % n1, "KChirpRows", "KChirpColInv<%d,true,false>" % n1]
    inv = "KChirpColInv<%d,false,true>" % n1 if c["entry"] == "kdv" else "KChirpColInv<%d,false,false>" % n1
    return ["KChirpColFwd<%d,false>" % n1, "KChirpRows", inv]


# bound constants (A, P) of tests/chirp_ref.err_bound, u (A log2 L + P Phi), one pair per form, each at most 10x the
# largest value measured on an MI355X (profiles/chirp_err.json): A from e / (u log2 L) on the tight grids (Phi ~ log2 L),
# P from e / (u Phi) on the wide ones
BOUND_RAW = (5.0, 0.2)    # raw values (chirpz): measured 0.59 (chirpz_N2_deg0) and 0.030 (rootfinder ring, N1 = 4)
BOUND_DFT = (10.0, 0.0)   # DFT mode (resample): 1.57 against the closed-form map, 4.14 against the oracle (every point,
                          # the oracle's own double-precision error included)
BOUND_NSE = (4.5, 0.25)   # NSE epilogue (plan, cache, tm): 0.46 (a, plan_4B_ab_N4_defocusing) and 0.0255 (a, wide grid)
BOUND_KDV = (0.5, 0.4)    # KdV epilogue (kdv): 0.051 (kdv_4B_cplx_N4); every KdV grid is tight, so P is set from
                          # e / (u Phi) there (0.049), an upper bound of the Phi term's share

_MID = 1 << 24
CASES = [
    # ---- fnft__poly_chirpz, raw values: every column length ----
    _c("chirpz_N2_deg0", "chirpz", 2, deg=0, M=5000),                              # M > deg + 1, deg = 0
    _c("chirpz_N2_tight_fit", "chirpz", 2, deg=5000, M=3192),                      # deg + M - 1 = L exactly
    _c("chirpz_N4_M7_ring_out", "chirpz", 4, deg=16000, M=7, ring=+1),             # M << deg, |A| = 1 + 1/deg
    _c("chirpz_N8_M_gt_deg", "chirpz", 8, deg=100, M=30001, wsign=-1),            # M > deg + 1, W below the axis
    _c("chirpz_N16_ring_in", "chirpz", 16, deg=40000, M=20001, ring=-1),          # |A| = 1 - 1/deg; R/BC edge 16|32
    _c("chirpz_N32", "chirpz", 32, deg=70001, M=50000, wsign=-1),
    _c("chirpz_N64_M_small", "chirpz", 64, deg=200000, M=1003),
    _c("chirpz_N128", "chirpz", 128, deg=300000, M=200001, ring=+1),
    _c("chirpz_N256", "chirpz", 256, deg=600000, M=300007, wsign=-1),             # R/BC edge 256|512
    _c("chirpz_N512", "chirpz", 512, deg=1500000, M=400001, K=6),
    _c("chirpz_N1024_M_gt_deg", "chirpz", 1024, deg=1000000, M=3000001, K=6, wsign=-1),
    _c("chirpz_N2048", "chirpz", 2048, deg=500000, M=7000001, K=6, ring=-1),
    _c("chirpz_N4096", "chirpz", 4096, deg=1 << 20, M=15000001, K=4),             # R/BC edge 4096|8192
    # L = 2^25 (the second master twiddle pair), deg ~ 2^24, deg + M - 1 = L exactly
    _c("chirpz_N8192_2p25_tight_fit", "chirpz", 8192, deg=_MID + (1 << 20), M=(1 << 25) - _MID - (1 << 20), K=4),
    # the root finder's rings (gridsearch_common): W = exp(i eps), eps = 2 pi/(M-1), A = 1 +- eps
    _c("chirpz_N2_rootfinder_ring_out", "chirpz", 2, deg=3000, M=4000, grid="wide", ring=+1),
    _c("chirpz_N4_rootfinder_ring_in", "chirpz", 4, deg=9000, M=6000, grid="wide", ring=-1),
    # ---- fnft__misc_resample: DFT mode, D in (L/4, L/2], odd / prime / not a power of two ----
    _c("resample_N2_D4093", "resample", 2, D=4093),
    _c("resample_N4_D8191", "resample", 4, D=8191),
    _c("resample_N8_D12000", "resample", 8, D=12000),
    _c("resample_N16_D32749", "resample", 16, D=32749),
    _c("resample_N32_D40001", "resample", 32, D=40001),
    _c("resample_N64_D131071", "resample", 64, D=131071),
    _c("resample_N128_D196613", "resample", 128, D=196613),
    _c("resample_N256_D524287", "resample", 256, D=524287, K=6),
    _c("resample_N512_D600001", "resample", 512, D=600001, K=6),
    _c("resample_N1024_D2097143", "resample", 1024, D=2097143, K=4),
    _c("resample_N2048_D3000017", "resample", 2048, D=3000017, K=4),
    _c("resample_N4096_D8388593", "resample", 4096, D=8388593, K=4),
    _c("resample_N8192_D9999991", "resample", 8192, D=9999991, K=4),              # D > 2^23: L = 2^25
    # ---- NSE epilogue on the plan's own tree: batch 3, XI not symmetric, M not a power of two ----
    _c("plan_MODAL_rho_N2", "plan", 2, disc="2SPLIT2_MODAL", D=1000, M=3001, batch=3, kappa=1,
       cstype="REFLECTION_COEFFICIENT"),
    _c("plan_4B_ab_N4_defocusing", "plan", 4, disc="2SPLIT4B", D=3000, M=4001, batch=3, kappa=-1, cstype="AB"),
    # a tree that ends in split levels: the root's finalize rides on KChirpColFwd (fin_max2), no launch of its own
    _c("plan_2A_both_N8_split_root", "plan", 8, disc="2SPLIT2A", D=16384, M=999, batch=3, kappa=1, cstype="BOTH",
       absent=["KFinalizeScales"]),
    _c("plan_MODAL_rho_N16_defocusing", "plan", 16, disc="2SPLIT2_MODAL", D=40000, M=20001, batch=3, kappa=-1,
       cstype="REFLECTION_COEFFICIENT"),
    _c("plan_4B_both_N2_wide", "plan", 2, disc="2SPLIT4B", D=2048, M=1500, batch=3, kappa=1, cstype="BOTH",
       grid="wide"),
    _c("plan_2A_both_N2_wide", "plan", 2, disc="2SPLIT2A", D=2000, M=1201, batch=3, kappa=-1, cstype="BOTH",
       grid="wide"),
    # ---- filter spectrum cache (v_mode 2) and caller transfer matrices (poly_tm, use_W) ----
    _c("cache_MODAL_N2", "cache", 2, disc="2SPLIT2_MODAL", D=2000, M=1001, batch=3, kappa=1, cstype="BOTH"),
    _c("tm_MODAL_both_N2_W7", "tm", 2, disc="2SPLIT2_MODAL", D=3000, M=2001, batch=2, W=7, cstype="BOTH"),
    _c("tm_4B_rho_N4_Wm5", "tm", 4, disc="2SPLIT4B", D=4000, M=3001, batch=2, W=-5,
       cstype="REFLECTION_COEFFICIENT"),
    # ---- KdV epilogue (KChirpColInv<N1, false, true>) at every column length: small D, large M ----
    _c("kdv_2A_real_N2", "kdv", 2, disc="2SPLIT2A", D=1000, M=5001, batch=2, real=1),
    _c("kdv_4B_cplx_N4", "kdv", 4, disc="2SPLIT4B", D=2000, M=9001, batch=2, real=0),
    _c("kdv_2A_cplx_N8", "kdv", 8, disc="2SPLIT2A", D=3000, M=25001, real=0),
    _c("kdv_3A_real_N16", "kdv", 16, disc="2SPLIT3A", D=4000, M=40001, real=1),
    _c("kdv_2A_real_N32", "kdv", 32, disc="2SPLIT2A", D=500, M=100001, real=1),
    _c("kdv_4B_real_N64", "kdv", 64, disc="2SPLIT4B", D=1000, M=200001, real=1),
    _c("kdv_1A_real_N128", "kdv", 128, disc="2SPLIT1A", D=1000, M=400001, real=1),
    _c("kdv_2A_cplx_N256", "kdv", 256, disc="2SPLIT2A", D=1000, M=800001, real=0),
    _c("kdv_2A_real_N512", "kdv", 512, disc="2SPLIT2A", D=1000, M=1600001, real=1),
    _c("kdv_4B_real_N1024", "kdv", 1024, disc="2SPLIT4B", D=1000, M=3000001, real=1, K=6),
    _c("kdv_2A_real_N2048", "kdv", 2048, disc="2SPLIT2A", D=1000, M=6000001, real=1, K=6),
    _c("kdv_4B_cplx_N4096", "kdv", 4096, disc="2SPLIT4B", D=1000, M=12000001, real=0, K=4),
    _c("kdv_2A_real_N8192", "kdv", 8192, disc="2SPLIT2A", D=1000, M=20000001, real=1, K=4),
]

EXCLUDED = {}

# degree per step of the schemes used above and in tests/handover_cases.py (nft_akns_degree)
DEG0 = {"2SPLIT2_MODAL": 1, "2SPLIT1A": 1, "2SPLIT2A": 1, "2SPLIT3A": 3, "2SPLIT3S": 2, "2SPLIT4A": 4, "2SPLIT4B": 2}


def case_ids():
    return [c["id"] for c in CASES]


def emu_args(c):
    """(entry, n, M, disc, batch, cstype, real) of emu_chirp_schedule for a case."""
    from fnft_amd.capi import CSTYPE, KDV_DISC, NSE_DISC
    e = c["entry"]
    if e == "chirpz":
        return 0, c["deg"], c["M"], 0, 1, -1, 0
    if e == "resample":
        return 1, c["D"], 0, 0, 1, -1, 0
    if e in ("plan", "cache", "tm"):
        return (3 if e == "tm" else 2), c["D"], c["M"], NSE_DISC[c["disc"]], c["batch"], CSTYPE[c["cstype"]], 0
    return 4, c["D"], c["M"], KDV_DISC[c["disc"]], c["batch"], 10, c["real"]


def rng(c, salt=0):
    return np.random.default_rng(zlib.crc32(c["id"].encode()) + salt)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def chirpz_inputs(c):
    """(p, A, W, m0): the polynomial (highest power first), the chirp constants, and the output index m0 at which the
    terms add up coherently (|X_m0| ~ mass, so that a relative error of the values is one of the metric too)."""
    deg, M, L = c["deg"], c["M"], ROW * c["N1"]
    r = rng(c)
    if c["grid"] == "wide":   # gridsearch_common: W = exp(i eps), A = (1 +- eps) exp(-i PHI0), PHI = [0, 2 pi]
        eps = 2 * np.pi / (M - 1)
        A = complex((1.0 + c.get("ring", 0) * eps) * np.cos(0.0), -(1.0 + c.get("ring", 0) * eps) * np.sin(0.0))
        W = complex(np.cos(eps), np.sin(eps))
    else:                     # Phi ~ log2 L: n^2 |arg W| / 2 <= log2 L / 2 and n |arg A| <= log2 L / 2 for n < L
        lg = np.log2(L)
        aw = c.get("wsign", 1) * lg / float(L - 1) ** 2
        aa = 0.5 * lg / float(L - 1)
        rad = 1.0 + c.get("ring", 0) / max(deg, 1)
        A = complex(rad * np.cos(aa), rad * np.sin(aa))
        W = complex(np.cos(aw), np.sin(aw))
    m0 = int(r.integers(0, M))
    n = np.arange(deg + 1, dtype=np.float64)
    lA, lW = np.log(A), np.log(W)
    w = r.uniform(0.5, 1.0, deg + 1) * (1 + 0.3 * (r.standard_normal(deg + 1) + 1j * r.standard_normal(deg + 1)))
    cn = w * np.exp(n * lA - n * float(m0) * lW)
    return cn[::-1].astype(np.complex128), A, W, m0


def out_points(c, M, extra=()):
    """K output indices: 0, M - 1, the given ones, and random ones (the last column block included)."""
    K = c["K"] or 12
    r = rng(c, 1)
    base = [0, M - 1] + [int(e) for e in extra]
    pts = set(base)
    while len(pts) < min(K, M):
        pts.add(int(r.integers(0, M)))
    return np.array(sorted(pts), np.int64)


def resample_inputs(c):
    """(q, eps_t, delta): random complex samples (every frequency present), a shift of 0.29 samples."""
    r = rng(c)
    D = c["D"]
    q = r.standard_normal(D) + 1j * r.standard_normal(D)
    eps_t = 0.1
    return q.astype(np.complex128), eps_t, 0.29 * eps_t


def tight_grid(L, D, M, deg1, xi0, nse):
    """(T, XI) with chirp phases Phi ~ log2 L and xi of order one: a short time step.  nse: arg A = -2 XI0 eps_t/deg1
    (fnft_nsev), else +2 XI0 eps_t/deg1 (fnft_kdvv); |arg V| = 2 eps_xi eps_t / deg1."""
    lg = np.log2(L)
    eps_t = 0.25 * lg * deg1 / (abs(xi0) * (L - 1))
    eps_xi = 0.5 * lg * deg1 / (float(L - 1) ** 2 * eps_t)
    T0 = -0.6 * eps_t * (D - 1)
    return (T0, T0 + eps_t * (D - 1)), (xi0, xi0 + eps_xi * (M - 1))


def grid(c):
    """(T, XI) of a plan / tm / kdv case."""
    deg1 = DEG0[c["disc"]]
    if c["grid"] == "wide":
        return (-20.0, 20.0), (-2.5, 3.1)
    nse = c["entry"] != "kdv"
    return tight_grid(ROW * c["N1"], c["D"], c["M"], deg1, -0.7 if nse else 0.7, nse)


def nse_signals(c, T, salt=0):
    """batch pulses of area 0.4 .. 0.6 (below the soliton threshold), chirped, shifted per signal."""
    D = c["D"]
    t = np.linspace(T[0], T[1], D)
    w = T[1] - T[0]
    out = []
    for k in range(c["batch"]):
        area = 0.4 + 0.1 * ((k + salt) % 3)
        a = 10.0 / w
        x = a * (t - T[0] - (0.45 + 0.05 * k) * w)
        q = area * a / np.pi / np.cosh(x) * np.exp(1j * (1.5 + 0.5 * k + salt) * x)
        out.append(q.astype(np.complex128))
    return out


def kdv_signals(c, T):
    """batch real pulses (sech^2 profile) of area 0.3 .. 0.5."""
    D = c["D"]
    t = np.linspace(T[0], T[1], D)
    w = T[1] - T[0]
    a = 10.0 / w
    return [((0.3 + 0.1 * (k % 3)) * a / 2.0 / np.cosh(a * (t - T[0] - (0.4 + 0.1 * k) * w)) ** 2).astype(np.complex128)
            for k in range(c["batch"])]


def tm_inputs(c):
    """batch transfer matrices [4, deg + 1] of exact doubles: identity-like diagonal, random off-diagonal entries."""
    deg = c["D"] * DEG0[c["disc"]]
    r = rng(c)
    tm = 0.3 / np.sqrt(deg + 1) * (r.standard_normal((c["batch"], 4, deg + 1))
                                   + 1j * r.standard_normal((c["batch"], 4, deg + 1)))
    tm[:, 0, 0] += 1.0
    tm[:, 3, -1] += 1.0
    return tm.astype(np.complex128)
