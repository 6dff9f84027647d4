"""Richardson extrapolation of the batched nsev plans in the CPU lane emulator, executing: the tree plan with
NftPlan::enable_richardson (child plan, KDsGather or the resampler's stride, KRichCombineCs), the discrete-spectrum plan
of nft_discspec_plan.h with its stage (guess plan and guess-free plan; coarse NftDiscSpecBatch, KRichMatchDs), and
KRichMatchDs alone on synthetic arrays.
Against the oracle's restatement of fnft_nsev with richardson_extrapolation_flag = 1, signal by signal.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import discspec_batch_cases as DC
import signals as S
from richardson_cases import CS_CASES, CS_M, CS_T, CS_TYPES, CS_XI, cs_signals
from oracle.oracle import NSE_DISC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_richardson.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p
sz = C.c_size_t
dbl = C.c_double

ORACLE_CS_REL = 1e-11       # test_gpu_parity.py: test_fnft_nsev_richardson_vs_oracle
ORACLE_BS_ABS = 1e-10       # test_discspec_batch_emu.py
ORACLE_NC_REL = 1e-8


def _P(a):
    return None if a is None else a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_richardson.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_arena.h", "nft_schemes.h", "nft_sub_grid.h", "nft_discspec.h",
                                             "nft_discspec_batch.h", "nft_discspec_search.h", "nft_discspec_plan.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_richardson.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_rich_contspec.argtypes = [sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.emu_rich_discspec.argtypes = [sz, sz, sz, C.c_int, C.c_int, sz, sz, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp,
                                    vp]
    L.emu_rich_match.argtypes = [sz, sz, dbl, dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.emu_rich_kernel_list.argtypes = [C.c_int, C.c_char_p, sz]
    return L


# ---- continuous spectrum ------------------------------------------------------------------------------------------
def run_contspec(emu, disc, q, cst, parts, richardson, kappa=1):
    B, D = q.shape
    out = np.full(B * parts * CS_M, np.nan + 0j)
    q0 = q.copy()
    rc = emu.emu_rich_contspec(D, CS_M, B, NSE_DISC[disc], kappa, cst, int(richardson), _P(q), _P(np.array(CS_T)),
                               _P(np.array(CS_XI)), _P(out))
    assert rc == 0, rc
    assert np.array_equal(q, q0)
    return out.reshape(B, parts, CS_M)


@pytest.mark.parametrize("disc,D,lo,hi", CS_CASES)
@pytest.mark.parametrize("cname,oname,cst,parts", CS_TYPES)
def test_contspec_vs_oracle_and_mask(emu, oracle, disc, D, lo, hi, cname, oname, cst, parts):
    q = cs_signals(D)
    on = run_contspec(emu, disc, q, cst, parts, True)
    off = run_contspec(emu, disc, q, cst, parts, False)
    for b in range(q.shape[0]):
        rc, ref = oracle.fnft_nsev(q[b], CS_T, CS_M, CS_XI, kappa=1, disc=disc, cstype=oname, richardson=True)
        rc0, ref0 = oracle.fnft_nsev(q[b], CS_T, CS_M, CS_XI, kappa=1, disc=disc, cstype=oname, richardson=False)
        assert rc == 0 and rc0 == 0
        ref, ref0 = ref.reshape(parts, CS_M), ref0.reshape(parts, CS_M)
        for j in range(parts):
            e = S.rel_err(on[b, j], ref[j])
            print(disc, D, cname, "signal", b, "part", j, "rel err vs oracle %.3e" % e)
            assert e < ORACLE_CS_REL, (b, j, e)
        changed = np.flatnonzero((on[b] != off[b]).any(axis=0))
        assert np.array_equal(changed, np.arange(lo, hi + 1)), changed
        assert np.array_equal(np.flatnonzero((ref != ref0).any(axis=0)), np.arange(lo, hi + 1))     # the oracle's own set


# ---- discrete spectrum --------------------------------------------------------------------------------------------
BSLOC = {"FAST_EIGENVALUE": 0, "NEWTON": 1, "SUBSAMPLE_AND_REFINE": 2}


def run_discspec(emu, disc, q, g, richardson, niter=10, bsfilt=2, dstype=2, want_nc=True, bsloc="NEWTON", Dsub=0, K=None):
    """g: the guesses of a guess plan; None: a guess-free plan with room for K bound states per signal."""
    B, D = q.shape
    K = g.shape[1] if g is not None else K
    bs = np.zeros((B, K), np.complex128)
    nc = np.zeros((B, 2 * K if dstype == 2 else K), np.complex128) if want_nc else None
    ko = np.zeros(B, np.uint64)
    st = np.zeros(B, np.int32)
    q0, g0 = q.copy(), None if g is None else g.copy()
    rc = emu.emu_rich_discspec(D, K, B, NSE_DISC[disc], BSLOC[bsloc], niter, Dsub, bsfilt, dstype, int(richardson), _P(q),
                               _P(np.array(DC.T)), _P(g), _P(bs), _P(nc), _P(ko), _P(st))
    assert rc == 0, rc
    assert np.array_equal(q, q0) and (g is None or np.array_equal(g, g0))
    return bs, nc, ko.astype(int), st


DS_CASES = [("2SPLIT4B", 300, 4, DC.PAIRS[1:4]), ("4SPLIT4B", 256, 3, DC.PAIRS[:5]), ("2SPLIT2_MODAL", 301, 4, DC.PAIRS[1:4])]


@pytest.mark.parametrize("disc,D,K,pairs", DS_CASES)
def test_discspec_vs_oracle(emu, oracle, disc, D, K, pairs):
    four = disc.startswith("4SPLIT")
    q, g = DC.batch(D, K, four, pairs)
    bs, nc, ko, st = run_discspec(emu, disc, q, g, True)
    bs0, nc0, ko0, st0 = run_discspec(emu, disc, q, g, False)
    assert not st.any() and not st0.any()
    assert np.array_equal(ko, ko0)
    for b in range(len(pairs)):
        rc, bs_o, nc_o, res_o = oracle.fnft_nsev_ds(q[b], DC.T, disc, bsloc="NEWTON", bsfilt="FULL", niter=10,
                                                    guesses=g[b], richardson=True)
        assert rc == 0
        k = bs_o.size
        assert ko[b] == k, (b, ko[b], bs[b], bs_o)
        e_bs = np.abs(bs[b, :k] - bs_o).max()
        e_nc = (np.abs(nc[b, :k] - nc_o) / np.abs(nc_o)).max()
        e_res = (np.abs(nc[b, K:K + k] - res_o) / np.abs(res_o)).max()
        print(disc, "signal", b, "K_out", k, "|bs - oracle| %.2e  nc rel %.2e  res rel %.2e" % (e_bs, e_nc, e_res))
        assert e_bs < ORACLE_BS_ABS
        assert e_nc < ORACLE_NC_REL and e_res < ORACLE_NC_REL
        assert np.isnan(bs[b, k:]).all() and np.isnan(nc[b, k:K]).all() and np.isnan(nc[b, K + k:]).all()
        # norming constants are not extrapolated; every bound state and residue is
        assert np.array_equal(nc[b, :k], nc0[b, :k])
        assert (bs[b, :k] != bs0[b, :k]).all() and (nc[b, K:K + k] != nc0[b, K:K + k]).all()


def test_discspec_output_layouts(emu):
    """RESIDUES is the residue half of BOTH; NORMING_CONSTANTS leaves the norming constants alone; without a norming
    array only the bound states are extrapolated -- all bitwise."""
    disc, D, K, pairs = DS_CASES[0]
    q, g = DC.batch(D, K, False, pairs)
    bs2, nc2, ko2, _ = run_discspec(emu, disc, q, g, True, dstype=2)
    bs1, nc1, ko1, _ = run_discspec(emu, disc, q, g, True, dstype=1)
    bs0, nc0, ko0, _ = run_discspec(emu, disc, q, g, True, dstype=0)
    bsn, _, kon, _ = run_discspec(emu, disc, q, g, True, dstype=2, want_nc=False)
    for bs, ko in ((bs1, ko1), (bs0, ko0), (bsn, kon)):
        assert np.array_equal(bs, bs2, equal_nan=True) and np.array_equal(ko, ko2)
    assert np.array_equal(nc1, nc2[:, K:], equal_nan=True)
    assert np.array_equal(nc0, nc2[:, :K], equal_nan=True)


SEARCH_CASES = [("2SPLIT4B", 256), ("4SPLIT4B", 128)]     # the coarse pass gathers; the coarse pass resamples


@pytest.mark.parametrize("disc,D", SEARCH_CASES)
def test_search_plan_vs_oracle(emu, oracle, disc, D):
    """The guess-free plan (SUBSAMPLE_AND_REFINE, FULL, niter = 10, BOTH) with the stage: the one statement of "fine
    pass, then stage" that the library runs, against the oracle's fnft_nsev with the flag, as sets per signal.
    Measured (2SPLIT4B / 4SPLIT4B): bound states within 6.7e-16 / 1.7e-15, norming constants 1.2e-15 / 1.7e-15, residues
    1.3e-14 / 8.6e-15, counts [2, 2, 3] -- what the shim's two former statements gave when transcribed over the emulator."""
    K, pairs = 4, DC.PAIRS[1:4]
    q = np.stack([DC.signal(D, A, c) for A, c in pairs])
    kw = dict(bsloc="SUBSAMPLE_AND_REFINE", K=K)
    bs, nc, ko, st = run_discspec(emu, disc, q, None, True, **kw)
    bs0, nc0, ko0, st0 = run_discspec(emu, disc, q, None, False, **kw)
    assert not st.any() and not st0.any()
    assert np.array_equal(ko, ko0)
    for b in range(len(pairs)):
        rc, bs_o, nc_o, res_o = oracle.fnft_nsev_ds(q[b], DC.T, disc, bsloc="SUBSAMPLE_AND_REFINE", bsfilt="FULL", niter=10,
                                                    richardson=True)
        assert rc == 0
        k = bs_o.size
        assert ko[b] == k, (b, ko[b], bs[b], bs_o)
        order = [int(np.abs(bs[b, :k] - x).argmin()) for x in bs_o]      # nearest pairs, one to one
        assert sorted(order) == list(range(k))
        e_bs = np.abs(bs[b, order] - bs_o).max()
        e_nc = (np.abs(nc[b, :K][order] - nc_o) / np.abs(nc_o)).max()
        e_res = (np.abs(nc[b, K:][order] - res_o) / np.abs(res_o)).max()
        print(disc, D, "signal", b, "K_out", k, "|bs - oracle| %.2e  nc rel %.2e  res rel %.2e" % (e_bs, e_nc, e_res))
        assert e_bs < ORACLE_BS_ABS
        assert e_nc < ORACLE_NC_REL and e_res < ORACLE_NC_REL
        # norming constants are not extrapolated; every bound state and residue is
        assert np.array_equal(nc[b, :k], nc0[b, :k])
        assert (bs[b, :k] != bs0[b, :k]).all() and (nc[b, K:K + k] != nc0[b, K:K + k]).all()


# ---- the match kernel alone ---------------------------------------------------------------------------------------
def match_ref(bs, bs_s, nc, res, nc_s, res_s, thr0, sn, sd):
    """oracle.py (fnft_nsev_ds, the loop over the fine bound states) on numpy arrays."""
    bs, res = bs.copy(), res.copy()
    for i in range(bs.size):
        loc, thr = bs_s.size, thr0
        for j in range(bs_s.size):
            e = abs(bs[i] - bs_s[j]) / abs(bs[i])
            if e < thr:
                thr, loc = e, j
        if loc < bs_s.size:
            bs[i] = (sn * bs[i] - bs_s[loc]) / sd
            ap_i = (sn * (nc[i] / res[i]) - (nc_s[loc] / res_s[loc])) / sd
            res[i] = nc[i] / ap_i
    return bs, res


def run_match(emu, K, fine, coarse, thr=0.05, sn=4.0, with_nc=True, status_s=None):
    """fine / coarse: per signal (bs, nc, res) arrays of the live entries.  Returns per signal (bs, res) of length K,
    the reference's, and the status words."""
    B = len(fine)
    nan = np.nan + 1j * np.nan
    bs = np.full((B, K), nan)
    bs_s = np.full((B, K), nan)
    nc = np.full((B, 2 * K), nan)
    nc_s = np.full((B, 2 * K), nan)
    kf = np.array([len(f[0]) for f in fine], np.uint64)
    ks = np.array([len(c[0]) for c in coarse], np.uint64)
    for b in range(B):
        for arr, arr_n, (v, n, r) in ((bs, nc, fine[b]), (bs_s, nc_s, coarse[b])):
            k = len(v)
            arr[b, :k], arr_n[b, :k], arr_n[b, K:K + k] = v, n, r
    res = np.full((B, K), 7.0 + 0j)
    st = np.zeros(B, np.int32)
    sts = np.zeros(B, np.int32) if status_s is None else np.array(status_s, np.int32)
    fine_in = bs.copy()
    tile = emu.emu_rich_match(K, B, thr, sn, sn - 1.0, _P(bs), _P(bs_s), _P(kf), _P(ks), _P(nc) if with_nc else None,
                              _P(nc_s) if with_nc else None, _P(res) if with_nc else None, _P(st), _P(sts))
    ref = [match_ref(np.array(f[0], np.complex128), np.array(c[0], np.complex128), np.array(f[1], np.complex128),
                     np.array(f[2], np.complex128), np.array(c[1], np.complex128), np.array(c[2], np.complex128),
                     thr, sn, sn - 1.0) for f, c in zip(fine, coarse)]
    return bs, res, ref, st, fine_in, nc, tile


def _close(a, b):
    return np.allclose(a, b, rtol=1e-14, atol=0.0)


def test_match_partner_rules(emu):
    """Signal 0: no coarse value within the threshold -- left alone.  Signal 1: two coarse values at the same distance --
    the lower index wins.  Signal 2: K_s = 0.  Signal 3: K = 0 (and a coarse status that must not be reported)."""
    K = 3
    f = [([1 + 2j, -1 + 1j], [2 + 1j, 3 - 1j], [0.5 + 0.25j, 1 - 1j])] * 3 + [([], [], [])]
    c = [([1.2 + 2j, -1 + 1.3j], [2 + 1j, 3 - 1j], [0.5 + 0.2j, 1 - 1.1j]),
         ([1.0078125 + 2j, 0.9921875 + 2j, -1 + 1.01j], [2.1 + 1j, 9 + 9j, 3 - 1.1j], [0.5 + 0.2j, 8 - 8j, 1 - 1.1j]),
         ([], [], []),
         ([1 + 2j], [1 + 1j], [1 - 1j])]
    bs, res, ref, st, fine_in, nc, _ = run_match(emu, K, f, c, thr=0.05, status_s=[0, 0, 0, 5])
    # distances of signal 1, entry 0: 2^-7 either way over |1 + 2i| -- equal, so index 0 is the partner
    assert abs((1 + 2j) - (1.0078125 + 2j)) == abs((1 + 2j) - (0.9921875 + 2j))
    for b in range(4):
        k = len(f[b][0])
        assert np.array_equal(bs[b, k:], fine_in[b, k:], equal_nan=True)
        assert np.array_equal(res[b, k:], nc[b, K + k:], equal_nan=True) and np.isnan(res[b, k:]).all()
        if k:
            assert _close(bs[b, :k], ref[b][0]) and _close(res[b, :k], ref[b][1])
    for b in (0, 2):      # nothing changed, bit for bit
        assert np.array_equal(bs[b], fine_in[b], equal_nan=True)
        assert np.array_equal(res[b], nc[b, K:], equal_nan=True)
    assert bs[1, 0] == (4.0 * (1 + 2j) - (1.0078125 + 2j)) / 3.0 and (bs[1] != fine_in[1])[:2].all()
    assert not st.any()
    # a coarse status is reported for a signal with bound states
    _, _, _, st, _, _, _ = run_match(emu, K, f[:1], c[:1], status_s=[5])
    assert st[0] == 5


def test_match_more_than_one_tile_and_pass(emu):
    """300 fine against 300 coarse values: two LDS tiles of coarse values, two passes of the 256 lanes; with and without
    the residue arrays."""
    K = 300
    rng = np.random.default_rng(7)
    v = rng.uniform(-3, 3, K) + 1j * rng.uniform(0.2, 3, K)
    n = rng.normal(size=K) + 1j * rng.normal(size=K)
    r = rng.normal(size=K) + 1j * rng.normal(size=K)
    perm = rng.permutation(K)
    vs = (v * (1 + 1e-3 * (rng.normal(size=K) + 1j * rng.normal(size=K))))[perm]
    vs[perm.tolist().index(17)] += 5.0            # entry 17 loses its partner
    ns = (n * (1 + 1e-3 * rng.normal(size=K)))[perm]
    rs = (r * (1 + 1e-3 * rng.normal(size=K)))[perm]
    bs, res, ref, st, fine_in, nc, tile = run_match(emu, K, [(v, n, r)], [(vs, ns, rs)], thr=0.02)
    assert K > tile and K > 256
    assert _close(bs[0], ref[0][0]) and _close(res[0], ref[0][1])
    assert bs[0, 17] == fine_in[0, 17] and res[0, 17] == nc[0, K + 17]
    assert (bs[0] != fine_in[0]).sum() == K - 1
    bs_only, res_only, _, _, _, _, _ = run_match(emu, K, [(v, n, r)], [(vs, ns, rs)], thr=0.02, with_nc=False)
    assert np.array_equal(bs_only, bs) and (res_only == 7.0).all()


# ---- kernel list ---------------------------------------------------------------------------------------------------
def test_third_aggregate(emu):
    """The new unit is listed in a third aggregate: its names are distinct from those of both existing ones, which keep
    their counts."""
    def names(which):
        buf = C.create_string_buffer(1 << 16)
        n = emu.emu_rich_kernel_list(which, buf, len(buf))
        v = [k.replace(" ", "") for k in buf.value.decode().split("\n") if k]
        assert n == len(v) == len(set(v)) and n > 0
        return v
    main, ext, ext2 = names(0), names(1), names(2)
    assert set(ext2) == {"KRichCombineCs", "KRichMatchDs"}
    assert len(main) == 258 and len(ext) == 3
    assert not set(ext2) & set(main) and not set(ext2) & set(ext)
    units = sorted(f[len("hip_kernels_"):-len(".hip")] for f in os.listdir(CSRC) if f.startswith("hip_kernels_"))
    assert len(units) == 25 and "richardson" in units
