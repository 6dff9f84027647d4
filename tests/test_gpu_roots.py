"""The two Ehrlich-Aberth root finders on the GPU, certified in extended precision (tests/roots_ref.py): the single one,
NftDiscSpec::roots behind fnft__poly_roots_fasteigen, and the batched, device-resident one of the guess-free discrete
spectrum, NftDiscSpecSearch::roots with the body_aberthb_* kernels, through the test seam fnft_amd__aberthb_roots.  Both
share the cores aberth_newton_core / aberth_sum_core / aberth_apply_core.

No reference root finder is involved and the pass condition has no measured constant: every value finite, Smith's
inclusion discs pairwise disjoint (one computed value per exact root, none missing, none doubled), and backward error
be <= 2 n u -- what every correctly rounded root meets (roots_ref.py).  A lost coefficient at a tile edge, a wrong
segment stride or join leaves be of order 1/n, ten or more orders above that.

Every test asserts that the path it names was taken, from the segments S of the plan and L = ceil8(ceil((m + 1) / S)),
the powers per Newton segment: S > 1 is a segmented sweep, L > 512 a Newton kernel with more than one coefficient tile,
n + 1 > 4096 a start kernel with log|c| and the hull in global memory.

Largest figures measured on an MI355X, per family: ROOTS_MEASURED below (every test prints its own figures; none of
them enters a bound).
"""
import numpy as np
import pytest

import roots_ref as R

pytestmark = pytest.mark.gpu
K_AB_SWEEPS = 80        # kAbSweeps, nft_kernels.h
K_AB_START_LDS = 4096   # kAbStartLds: coefficients body_aberthb_start keeps in LDS
NEWTON_TILE = 512       # coefficients per tile of the Newton kernel (KAberthNewton, KAberthBNewton)
# family: (largest be/(n u), smallest disc gap, largest r/|z|) on an MI355X; the bound on be/(n u) is 2 for all of them
ROOTS_MEASURED = {
    "single, Kac n 127 .. 513": (0.0863, 3.6e-3, 1.17e-13),
    "single, Kac n 8200": (0.0145, 1.41e-4, 2.2e-12),
    "single, Kac scaled out / in, n 129 and 513": (0.0797, 1.67e-3, 1.1e-13),
    "single, two_scale(200, 313)": (0.548, 1.26e-2, 1.02e-13),
    "batched, Kac and scaled Kac, n 129 .. 257": (0.0975, 2.48e-3, 5.08e-14),
    "batched, two_scale(100, 157)": (0.588, 2.51e-2, 5.49e-14),
    "batched, zero ends in n 160": (0.425, 4.81e-2, 1.23e-14),
    "batched, Kac n 520 x 700": (0.0585, 5.02e-4, 1.19e-13),
    "batched, Kac n 4095 and 4096": (0.025, 2.54e-4, 1.09e-12),
}
# Before the cores formed |c| and |p| by hypot, the single finder left be/(n u) = 6.0e4 on kac_scaled(513, +1) (|p|^2
# underflowed in the test against the evaluation noise) and 8.6e12 with overlapping discs on kac_scaled(513, -1) (|c|^2
# overflowed the error scale), both with rc = 0: test_single_kac_scaled found it.


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import capi as c
    c.load()
    c.silence_errors()
    return c


def single_first_S(n):
    """Segments of the single finder's first sweeps, while every estimate still moves (NftDiscSpec::roots: 2048
    workgroups per launch, at most 16 segment values per estimate)."""
    if n < 128:
        return 1
    gx = (n + 255) // 256
    return max(1, min((2048 + gx - 1) // gx, 64, 16))


def run_single(capi, label, c):
    c0 = c.copy()
    rc, z = capi.poly_roots_fasteigen(c)
    assert rc == 0, capi.last_error()
    assert np.array_equal(c, c0)
    return R.certify(label, c, z), z


# ---- the single finder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [127, 128, 129, 255, 256, 257, 511, 512, 513])
def test_single_kac_edges(capi, n):
    """Degrees at the edges of the segmentation threshold (128) and of the 256-lane workgroups."""
    S = single_first_S(n)
    print("n", n, "first sweeps: S", S, "L", R.seg_len(n, S))
    assert (S > 1) == (n >= 128)
    run_single(capi, "single kac n %d" % n, R.kac(n, 1000 + n))


@pytest.mark.parametrize("n", [129, 513])
@pytest.mark.parametrize("s", [+1, -1])
def test_single_kac_scaled(capi, n, s):
    """Roots around |z| = 2 (s = +1: the 1/z branch) or around 1/2 (c_powi on small |x|^L).  A Kac polynomial has a few
    roots well off the unit circle, so a scaled one may keep a few on the other side of it."""
    c = R.kac_scaled(n, 2000 + n, s)
    _, z = run_single(capi, "single kac_scaled n %d s %+d" % (n, s), c)
    assert ((np.abs(z) > 1) if s > 0 else (np.abs(z) < 1)).mean() > 0.9


def test_single_two_scale(capi):
    """Two hull slopes, 200 roots at |z| = 0.4 and 313 at 2.5: both branches in one workgroup."""
    c = R.two_scale(200, 313)
    _, z = run_single(capi, "single two_scale(200, 313)", c)
    assert (np.abs(z) < 1).sum() == 200 and (np.abs(z) > 1).sum() == 313


def test_single_kac_8200_two_tiles(capi):
    """n = 8200: the first sweeps have S = 16 and L = 520 > 512, so the Newton kernel walks two coefficient tiles."""
    n = 8200
    S = single_first_S(n)
    assert S == 16 and R.seg_len(n, S) == 520 > NEWTON_TILE
    run_single(capi, "single kac n 8200", R.kac(n, 8200))


# ---- the batched finder alone ----------------------------------------------------------------------------------------
def run_batched(capi, polys):
    polys = np.ascontiguousarray(polys, np.complex128)
    p0 = polys.copy()
    rc, z, mdeg, st, wn, sw, S = capi.aberthb_roots(polys)
    assert rc == 0, capi.last_error()
    assert np.array_equal(polys, p0)
    assert not st.any() and not wn.any()
    assert (sw > 0).all() and (sw < K_AB_SWEEPS).all()
    return z, mdeg, sw, S


def test_batched_129_three_hulls(capi):
    """n = 129, batch 3: Kac, scaled out, scaled in -- three different hulls in one launch, segmented."""
    n = 129
    polys = np.stack([R.kac(n, 129), R.kac_scaled(n, 130, +1), R.kac_scaled(n, 131, -1)])
    z, mdeg, sw, S = run_batched(capi, polys)
    print("S", S, "L", R.seg_len(n, S), "sweeps", sw)
    assert S > 1 and (mdeg == n).all()
    assert (np.abs(z[1]) > 1).mean() > 0.9 and (np.abs(z[2]) < 1).mean() > 0.9
    for b, name in enumerate(("kac", "scaled out", "scaled in")):
        R.certify("batched n 129 %s" % name, polys[b], z[b])


def test_batched_257_five(capi):
    """n = 257, batch 5: two_scale(100, 157), two Kac, the two scalings; two workgroups per signal and segment."""
    n = 257
    polys = np.stack([R.two_scale(100, 157), R.kac(n, 257), R.kac(n, 258), R.kac_scaled(n, 259, +1),
                      R.kac_scaled(n, 260, -1)])
    z, mdeg, sw, S = run_batched(capi, polys)
    print("S", S, "L", R.seg_len(n, S), "sweeps", sw)
    assert S > 1 and (mdeg == n).all()
    assert (np.abs(z[3]) > 1).mean() > 0.9 and (np.abs(z[4]) < 1).mean() > 0.9
    assert (np.abs(z[0]) < 1).sum() == 100 and (np.abs(z[0]) > 1).sum() == 157
    for b, name in enumerate(("two_scale(100, 157)", "kac", "kac", "scaled out", "scaled in")):
        R.certify("batched n 257 %s" % name, polys[b], z[b])


def test_batched_160_zero_ends_mixed_degrees(capi):
    """n = 160, batch 3: reduced degrees 130 (segmented), 96 (not segmented: below 128) and 160 in one plan."""
    n, c = 160, 0.5 + 0.3j
    shapes = [(10, 130, 20), (40, 96, 24)]
    polys = np.stack([R.zero_ends(nl, m, nt, c) for nl, m, nt in shapes] + [R.kac(n, 160)])
    z, mdeg, sw, S = run_batched(capi, polys)
    print("S", S, "sweeps", sw)
    assert S > 1
    assert list(mdeg) == [130, 96, 160]
    for b, (nl, m, nt) in enumerate(shapes):
        R.certify_with_ends("batched n 160 zero ends %s" % ((nl, m, nt),), polys[b], z[b])
        exact = c ** (1.0 / m) * np.exp(2j * np.pi * np.arange(m) / m)
        err = max(np.abs(z[b, :m] - e).min() for e in exact)
        print("signal", b, "m", m, "max |root - exact|", err)
        assert err < 1e-13          # the emulator test's bound (test_discspec_search_emu.py)
    R.certify("batched n 160 kac", polys[2], z[2])


def test_batched_520_two_tiles_700(capi):
    """n = 520, batch 700: S = 1 and L = 528, so the Newton kernel walks two tiles, the tail tile with two blocks of
    eight.  Seven distinct polynomials, slot b holds number b % 7: the first and the last seven slots are certified, and
    every slot equals slot b % 7 bit for bit (one plan, one S, the same arithmetic per estimate)."""
    n, B = 520, 700
    seven = np.stack([R.kac(n, 520 + i) for i in range(7)])
    polys = seven[np.arange(B) % 7]
    z, mdeg, sw, S = run_batched(capi, polys)
    L = R.seg_len(n, S)
    print("S", S, "L", L, "sweeps of the seven", sw[:7])
    assert S == 1 and L == 528 > NEWTON_TILE and (L // 8) % (NEWTON_TILE // 8) == 2
    assert (mdeg == n).all()
    for b in list(range(7)) + list(range(B - 7, B)):
        R.certify("batched n 520 slot %d" % b, polys[b], z[b])
    differ = [b for b in range(B) if z[b].tobytes() != z[b % 7].tobytes() or sw[b] != sw[b % 7]]
    assert not differ, differ[:20]


@pytest.mark.parametrize("n", [4095, 4096])
def test_batched_start_kernel_lds_edge(capi, n):
    """n = 4095: log|c| and the hull fill the start kernel's LDS arrays; n = 4096: they live in global memory, signal 1
    at its stride."""
    polys = np.stack([R.kac(n, n), R.kac(n, n + 7)])
    assert (n + 1 > K_AB_START_LDS) == (n == 4096)
    z, mdeg, sw, S = run_batched(capi, polys)
    print("S", S, "L", R.seg_len(n, S), "sweeps", sw)
    assert S > 1 and (mdeg == n).all()
    for b in range(2):
        R.certify("batched n %d signal %d" % (n, b), polys[b], z[b])
