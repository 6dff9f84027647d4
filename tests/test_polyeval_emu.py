"""The polynomial evaluation kernels (KPolyEval, KPolyJoin) and the plan logic of fnft_amd_nsev_eval_device
(NftPlan::run_eval) in the CPU lane emulator, executing.  No GPU needed.

Every figure is e = |got - long double| / scale (tests/polyval_ref.py) and every test asserts the MAXIMUM over all of its
points: e <= max(MARGIN e_dbl, FLOOR), e_dbl being the same figure of the reference's formula run in double.  The NSE
layer applies the formulas to the matrix the emulated plan itself exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polyeval_cases as PC
import polyval_ref as PR
from fnft_amd.capi import NSE_DISC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_polyeval.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")
vp = C.c_void_p
sz = C.c_size_t


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_polyeval.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in ("dev_compat.h", "fft_dev.h", "nft_kernels.h", "nft_real.h", "nft_dispatch.h",
                                             "nft_kernel_list.h", "nft_plan.h", "nft_chirp.h", "nft_twiddles.h",
                                             "nft_arena.h", "nft_schemes.h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_polyeval.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_polyeval.argtypes = [sz, sz, sz, vp, sz, sz, sz, vp, sz, vp, vp, C.c_int, vp]
    L.emu_nsev_eval.argtypes = [sz, sz, sz, C.c_int, C.c_int, vp, vp, vp, vp, sz, sz, C.c_int, C.c_int, C.c_int, vp, vp,
                                vp, vp, C.c_char_p, sz]
    L.emu_ext_kernel_list.argtypes = [C.c_int, C.c_char_p, sz]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def poly_run(emu, deg, nz, batch=1, npoly=1, shared=True, pad=0, deriv=True, S=0, key=()):
    """One emu_polyeval call on random coefficients and PC.points; asserts the bound for every polynomial and returns
    (S, L) of the launch.  pad: extra elements in every stride."""
    ps, bs = deg + 1 + pad, npoly * (deg + 1 + pad) + pad
    zs = 0 if shared else nz + pad
    p = PC.coefficients(batch * bs, deg, nz, batch, npoly, *key)
    z = PC.points((1 if shared else batch) * (nz + pad), deg, *key)
    val = np.full(batch * npoly * nz, np.nan + 0j)
    der = np.full(batch * npoly * nz, np.nan + 0j) if deriv else None
    seg = np.zeros(2, np.int64)
    rc = emu.emu_polyeval(deg, npoly, batch, _p(p), ps, bs, nz, _p(z), zs, _p(val), _p(der), S, _p(seg))
    assert rc == 0
    val = val.reshape(batch, npoly, nz)
    worst = {}
    for b in range(batch):
        zb = z[b * zs:b * zs + nz]
        for j in range(npoly):
            c = p[b * bs + j * ps:b * bs + j * ps + deg + 1]
            f = PR.poly_errors(c, zb, val[b, j], der.reshape(batch, npoly, nz)[b, j] if deriv else None)
            for k, v in f.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("deg %d nz %d batch %d npoly %d S %d L %d:" % (deg, nz, batch, npoly, seg[0], seg[1]),
          " ".join("%s %.2f u" % (k, v / PR.U) for k, v in sorted(worst.items())))
    PR.check_poly(worst)
    return int(seg[0]), int(seg[1])


@pytest.mark.parametrize("deg", PC.DEGS)
@pytest.mark.parametrize("nz", PC.NZS)
def test_degrees_and_point_counts(emu, deg, nz):
    S, L = poly_run(emu, deg, nz)
    assert L % 8 == 0 and S * L >= deg + 1 and (S - 1) * L < deg + 1


@pytest.mark.parametrize("deg,nz", [(0, 65), (9, 1), (PC.TILE + 1, 257)])
def test_values_only(emu, deg, nz):
    poly_run(emu, deg, nz, deriv=False)


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("npoly", (1, 2))
@pytest.mark.parametrize("shared", (True, False))
@pytest.mark.parametrize("pad,deriv", [(0, True), (3, True), (3, False)])
def test_layouts(emu, batch, npoly, shared, pad, deriv):
    poly_run(emu, 13, 65, batch=batch, npoly=npoly, shared=shared, pad=pad, deriv=deriv)


@pytest.mark.parametrize("deg,S,L", [(2 * PC.TILE + 5, 1, 1032), (2 * PC.TILE + 5, 2, 520), (2 * PC.TILE + 5, 3, 344),
                                     (21, 3, 8), (5, 2, 8), (PC.TILE, 3, 176)])
def test_forced_segments(emu, deg, S, L):
    """S segments of L powers: a ragged last segment (1030 = 2 * 344 + 342; 22 = 8 + 8 + 6; 513 = 2 * 176 + 161), and
    deg < L, where the second segment holds no coefficient at all."""
    assert poly_run(emu, deg, 65, batch=2, npoly=2, shared=False, S=S) == (S, L)
    poly_run(emu, deg, 63, deriv=False, S=S)


def test_ext_units(emu):
    """FA_EXT_UNITS holds the units added after FA_ALL_UNITS' count was pinned: names distinct, non-empty, and none of
    them in FA_ALL_UNITS (the list emu_kernel_list prints)."""
    def names(which):
        buf = C.create_string_buffer(1 << 16)
        n = emu.emu_ext_kernel_list(which, buf, len(buf))
        v = [k.replace(" ", "") for k in buf.value.decode().split("\n") if k]
        assert n == len(v) == len(set(v)) and n > 0
        return v
    ext, main = names(1), names(0)
    assert set(ext) == {"KPolyEval<false>", "KPolyEval<true>", "KPolyJoin"}
    assert len(main) == 258 and not set(ext) & set(main)


# ---- NSE layer ---------------------------------------------------------------------------------------------------
T = (-2.0, 2.0)


def nse_run(emu, disc, D, kappa, lam, batch=1, per_signal=False, deriv=True, S=0, M=0, XI=(-1.0, 1.0), reps=1):
    """One emu_nsev_eval call.  lam: [n] shared or [batch, n].  dict(out [batch, parts*n], tm, W, cs, names)."""
    lam = np.ascontiguousarray(lam, np.complex128)
    n = lam.shape[-1]
    deg = D * PC.UPS[disc] * PC.DEG0[disc]
    q = PC.nse_signal(D, T, batch, disc, kappa)
    out = np.full(batch * (4 if deriv else 2) * n, np.nan + 0j)
    cs = np.zeros(batch * 2 * max(M, 1), np.complex128)
    tm = np.zeros(batch * 4 * (deg + 1), np.complex128)
    W = np.zeros(batch, np.int32)
    Ta, Xa = np.array(T, np.float64), np.array(XI, np.float64)
    buf = C.create_string_buffer(1 << 14)
    rc = emu.emu_nsev_eval(D, M, batch, NSE_DISC[disc], kappa, _p(q), _p(Ta), _p(Xa), _p(lam), n, n if per_signal else 0,
                           int(deriv), S, reps, _p(out), _p(cs), _p(tm), _p(W), buf, len(buf))
    assert rc == 0, rc
    parts, cur = {}, None
    for k in buf.value.decode().split("\n"):
        if k.startswith("--"):
            cur = parts.setdefault(k[2:], [])
            cur.append([])
        elif k and cur is not None:
            cur[-1].append(k.replace(" ", ""))
    return dict(out=out.reshape(batch, -1), tm=tm.reshape(batch, 4, deg + 1), W=W, cs=cs.reshape(batch, -1), names=parts)


def nse_check(tag, r, disc, D, lam, deriv):
    consts = PR.nse_consts(T, D, PC.DEG0[disc], PC.UPS[disc], disc in ("2SPLIT2_MODAL", "2SPLIT2A"))
    lam = np.asarray(lam)
    worst = dict(e=0.0, e_dbl=0.0)
    for b in range(r["out"].shape[0]):
        f = PR.nse_errors(r["tm"][b], r["W"][b], lam if lam.ndim == 1 else lam[b], consts, r["out"][b], deriv)
        worst = dict(e=max(worst["e"], f["e"]), e_dbl=max(worst["e_dbl"], f["e_dbl"]))
    print(tag, "W", r["W"], "e %.2f u  e_dbl %.2f u" % (worst["e"] / PR.U, worst["e_dbl"] / PR.U))
    assert worst["e"] <= PR.bound(worst["e_dbl"], PR.FLOOR_NSE), (tag, worst)


NSE_CASES = [("2SPLIT2_MODAL", 16, 1), ("2SPLIT4B", 32, 1), ("4SPLIT4A", 16, 1), ("2SPLIT4B", 32, -1)]


@pytest.mark.parametrize("disc,D,kappa", NSE_CASES)
@pytest.mark.parametrize("kind", ("real", "complex"))
def test_nse_values_and_derivatives(emu, disc, D, kappa, kind):
    lam = PC.lambdas(70, T, kind, disc)
    r = nse_run(emu, disc, D, kappa, lam)
    nse_check("%s D %d kappa %d %s" % (disc, D, kappa, kind), r, disc, D, lam, True)
    # the matrix is exported once, by the evaluation; two launches evaluate
    assert r["names"]["eval"] == [[k for k in r["names"]["eval"][0] if not k.startswith("KPoly")]
                                  + ["KPolyEval<true>", "KPolyJoin"]]
    assert r["names"]["eval"][0].count("KExportTm") == 1


def test_nse_batch_per_signal_values_only_segments(emu):
    """Three signals with their own points, values only, two segments (deg 64 < 2 L: ragged), evaluated twice: the second
    call launches the two kernels and nothing else (no export, no root pass)."""
    disc, D = "2SPLIT4B", 32
    lam = np.array([PC.lambdas(65, T, "complex", b) for b in range(3)])
    r = nse_run(emu, disc, D, 1, lam, batch=3, per_signal=True, deriv=False, S=2, reps=2)
    nse_check("batch 3 per-signal", r, disc, D, lam, False)
    assert r["names"]["eval"][1] == ["KPolyEval<false>", "KPolyJoin"]


@pytest.mark.parametrize("disc,D", [("2SPLIT2_MODAL", 16), ("4SPLIT4A", 16)])
def test_nse_on_the_plans_own_grid(emu, disc, D):
    """Real lambda on the xi-grid of the plan, upsampling 1 and 2: the evaluation against the chirp transform's contspec
    of type AB (polyval_ref.own_grid_check)."""
    M, XI = 24, (-1.5, 2.0)
    xi = XI[0] + (XI[1] - XI[0]) / (M - 1) * np.arange(M)
    r = nse_run(emu, disc, D, 1, xi.astype(np.complex128), deriv=False, M=M, XI=XI)
    nse_check("own grid " + disc, r, disc, D, xi, False)
    consts = PR.nse_consts(T, D, PC.DEG0[disc], PC.UPS[disc], disc in ("2SPLIT2_MODAL", "2SPLIT2A"))
    PR.own_grid_check(r["tm"][0], r["W"][0], consts[4], T, XI, M, D, consts, r["out"][0], r["cs"][0])


def test_partials_do_not_grow_when_n_shrinks(emu):
    """A plan sizes its segment partials by polyeval_partials, the HIP back end aims at 2048 workgroups: walking n down
    across the multiples of 256 -- where S doubles as long as a segment keeps its 1024 powers (deg = 2^20, two
    polynomials; deg = 2^18, eight) -- the size never grows, and it always holds the S * jobs * n the launch writes."""
    emu.emu_polyeval_sizes.argtypes = [sz, sz, sz, sz, vp]
    for deg, jobs in ((1 << 20, 2), (1 << 18, 8), (8192, 4), (1 << 16, 128)):
        prev, seen = None, set()
        for n in list(range(1300, 0, -1)):
            o = np.zeros(3, np.int64)
            emu.emu_polyeval_sizes(deg, n, jobs, 2048, _p(o))
            S, L, part = (int(x) for x in o)
            seen.add(S)
            assert L % 8 == 0 and S * L >= deg + 1 and (S - 1) * L < deg + 1
            assert S * jobs * n <= part, (deg, jobs, n, S, part)
            assert prev is None or part <= prev, (deg, jobs, n, part, prev)
            prev = part
        if deg == 1 << 20:
            assert len(seen) >= 3, seen     # S did change on the way down: 257, 342, 512, 1024
