"""The batched Ehrlich-Aberth root finder (NftDiscSpecSearch::roots, the body_aberthb_* kernels and the cores
aberth_newton_core / aberth_sum_core / aberth_apply_core they share with the single finder) in the CPU lane emulator,
certified in extended precision by tests/roots_ref.py -- and that certificate's own tests.  No GPU needed.

The pass condition has no measured constant (roots_ref.py): every value finite, Smith's discs pairwise disjoint, and
backward error <= 2 n u.  Figures of the present kernels in the emulator, for the record (each test prints its own):
max be/(n u) 0.04 - 0.12 on the Kac trio of degree 129 and 0.52 on two_scale(60, 100); smallest disc gap 0.007 - 0.04;
max r/|z| 5.3e-14."""
import ctypes as C

import numpy as np
import pytest

import roots_ref as R
from test_discspec_search_emu import emu  # noqa: F401  (the emulator library, built by the same staleness rule)

vp = C.c_void_p


def _P(a):
    return a.ctypes.data_as(vp)


def run_emu(emu, polys):  # noqa: F811
    """polys[batch, n + 1] -> (roots[batch, n], mdeg, status, warnings, sweeps, S) of the emulator's seam."""
    polys = np.ascontiguousarray(polys, np.complex128)
    B, n = polys.shape[0], polys.shape[1] - 1
    tm = R.tm_blocks(polys)
    tm0 = tm.copy()
    z = np.zeros((B, n), np.complex128)
    mdeg, st, wn, sw = (np.zeros(B, np.int32) for _ in range(4))
    sz = np.zeros(1, np.uint64)
    assert emu.emu_aberthb_roots(n, B, _P(tm), _P(z), _P(mdeg), _P(st), _P(wn), _P(sw), _P(sz)) == 0
    assert np.array_equal(tm, tm0)
    return z, mdeg, st, wn, sw, int(sz[0])


def check_words(mdeg, st, wn, sw, m):
    assert not st.any() and not wn.any()
    assert (mdeg == m).all() and (sw > 0).all() and (sw < 80).all()      # kAbSweeps


def test_kac_trio_129(emu):  # noqa: F811
    """Three different hulls in one launch: Kac, scaled out (the 1/z branch), scaled in."""
    n = 129
    polys = np.stack([R.kac(n, 129), R.kac_scaled(n, 130, +1), R.kac_scaled(n, 131, -1)])
    z, mdeg, st, wn, sw, S = run_emu(emu, polys)
    print("segments", S, "L", R.seg_len(n, S), "sweeps", sw)
    assert S > 1
    check_words(mdeg, st, wn, sw, n)
    assert (np.abs(z[1]) > 1).mean() > 0.9 and (np.abs(z[2]) < 1).mean() > 0.9
    for b, name in enumerate(("kac", "kac scaled out", "kac scaled in")):
        R.certify("emu n 129 %s" % name, polys[b], z[b])


def test_two_scale_60_100(emu):  # noqa: F811
    """Two hull slopes, roots on both sides of the unit circle, four non-zero coefficients."""
    c = R.two_scale(60, 100)
    z, mdeg, st, wn, sw, S = run_emu(emu, c[None, :])
    print("segments", S, "L", R.seg_len(160, S), "sweeps", sw)
    assert S == 8
    check_words(mdeg, st, wn, sw, 160)
    assert (np.abs(z[0]) < 1).sum() == 60 and (np.abs(z[0]) > 1).sum() == 100
    R.certify("emu two_scale(60, 100)", c, z[0])


# ---- the certificate's own tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 257])
def test_bound_discriminates_numpy_roots(n):
    """np.roots (LAPACK's QR on the companion matrix, backward stable in the matrix norm) finds every root -- the discs
    are disjoint -- but its values are not the nearest doubles: be is hundreds of u, above 2 n u."""
    c = R.kac(n, n)
    cert = R.certificate(c, np.roots(c))
    print("np.roots, Kac n %d: max be/(n u) %.4g  smallest gap %.4g  max r/|z| %.4g" % ((n,) + R.figures(cert)))
    assert cert["finite"] and cert["gap"] > 0
    assert np.max(cert["be"]) > R.be_bound(n)
    assert R.failures(cert) == ["backward error %.3e n u > 2 n u" % (np.max(cert["be"]) / (n * R.U))]


def _polished(c):
    """Roots of c to the last bit or two: np.roots, then Newton steps in long double, rounded to double."""
    z = np.roots(c).astype(R.CLD)
    cl = c.astype(R.CLD)
    dl = cl[:-1] * np.arange(c.size - 1, 0, -1).astype(R.LD)
    for _ in range(4):
        z = z - np.polyval(cl, z) / np.polyval(dl, z)
    return z.astype(np.complex128)


def test_certificate_accepts_rounded_roots_and_rejects_defects():
    """Exact roots rounded to double pass (with be well below the bound: the nearest double is within u |z|); a root
    replaced by a copy of another one fails disjointness; a root moved by 1e-9 |z| fails the backward error."""
    n = 129
    c = R.kac(n, 7)
    z = _polished(c)
    f = R.certify("long-double Newton, Kac n 129", c, z)
    assert f[0] <= 1.0
    dup = z.copy()
    dup[5] = dup[17]
    cert = R.certificate(c, dup)
    assert not cert["gap"] > 0 and any("disjoint" in s for s in R.failures(cert))
    moved = z.copy()
    moved[40] *= 1.0 + 1e-9
    cert = R.certificate(c, moved)
    assert cert["be"][40] > R.be_bound(n) and any("backward" in s for s in R.failures(cert))
    assert np.delete(cert["be"], 40).max() <= R.be_bound(n)
    bad = z.copy()
    bad[3] = np.nan
    assert "not finite" in R.failures(R.certificate(c, bad))


def test_outside_branch_matches_inside():
    """The same values scaled by 4 against the coefficients scaled exactly: the 1/z branch gives the ratio of the z
    branch, and radii 4 times as large."""
    n = 65
    c_in, c_out = R.kac_scaled(n, 3, -1), R.kac_scaled(n, 3, +1)
    z = _polished(c_in) * (1.0 + 1e-12)       # off the roots by far more than the long-double rounding of either branch
    a, b = R.certificate(c_in, z), R.certificate(c_out, 4.0 * z)
    assert (np.abs(z) < 1).all() and (np.abs(4.0 * z) > 1).all()
    assert a["be"].min() > 1e3 * n * 2.0 ** -64
    assert np.allclose(a["be"], b["be"], rtol=1e-3, atol=0) and np.allclose(4.0 * a["r"], b["r"], rtol=1e-3, atol=0)


def test_families():
    assert R.trim(R.zero_ends(10, 130, 20, 0.5 + 0.3j))[:3] == (10, 130, 20)
    c = R.two_scale(3, 4)
    assert c.size == 8 and np.count_nonzero(c) == 4
    k, ko = R.kac(9, 1), R.kac_scaled(9, 1, +1)
    assert ko[0] == k[0] * 2.0 ** -9 and ko[-1] == k[-1]
    assert [R.seg_len(8200, 16), R.seg_len(520, 1), R.seg_len(129, 16)] == [520, 528, 16]
