"""Extended-precision certificate for a computed set of polynomial roots (helper module, not a test).

No reference root finder is involved: the roots are judged against the polynomial itself, whose double coefficients
c (highest power first, degree n, c[0] != 0 != c[n]) are taken as exact.  For computed roots z_0 .. z_{n-1}:

  backward error   be_k = |p(z_k)| / sum_j |c_j| |z_k|^j, by Horner's scheme in np.clongdouble -- in z where |z| <= 1,
                   on the reversed polynomial in x = 1/z where |z| > 1 (p(z) = z^n q(x): the same ratio, no overflow)
  Smith's radii    r_k = n |p(z_k)| / (|c_0| prod_{j != k} |z_k - z_j|), formed through sums of logarithms.  The union
                   of the discs |z - z_k| <= r_k holds every root of p, and a disc disjoint from all others holds
                   exactly one (B. T. Smith, J. ACM 17 (1970), 661-674)
  gap              the smallest |z_k - z_j| - r_k - r_j over all pairs, and max r_k / |z_k|

Pass condition (certified): all n values finite, gap > 0 -- one computed value per exact root, none missing and none
doubled -- and be_k <= 2 n u, u = 2^-53.  The last is no property of a code under test: a double within 2 u |z| of an
exact root zeta (the nearest double is within u |z|) has |p(z)| <= 2 u |z| |p'| <= 2 n u sum_j |c_j| |z|^j, so every
correctly rounded root meets it, while a defect in an evaluation (a lost coefficient, a wrong segment join) leaves be of
order 1/n.

Accuracy of the certificate itself: Horner's scheme in long double (64-bit significand) errs by at most 2 n 2^-64 of
the denominator, and 1/z by 2^-64 relative, which moves q by at most n 2^-64 of it: 2^-10 of the bound together.  The
pairwise distances run in double -- each |z_k - z_j| is good to 2^-52 relative, the sum of n logarithms to n 2^-52
absolute, nothing next to the orders of magnitude between a radius and a gap.  They are chunked over rows so that
memory stays bounded at n = 8200.

The polynomial families of tests/test_gpu_roots.py and tests/test_roots_emu.py live here too, all deterministic.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
CLD = np.clongdouble
_CHUNK = 1 << 21   # pairwise distances per chunk (x 8 bytes x a few temporaries)


# ---- the certificate ---------------------------------------------------------------------------------------------
def _horner(c, x):
    """(p(x), sum_j |c_j| |x|^j) for c highest power first, in long double; x: clongdouble vector."""
    ax = np.abs(x)
    p = np.zeros(x.shape, CLD)
    s = np.zeros(x.shape, LD)
    for cj, aj in zip(c.astype(CLD), np.abs(c.astype(CLD))):
        p = p * x + cj
        s = s * ax + aj
    return p, s


def certificate(c, z):
    """c: n + 1 coefficients, highest power first, both end coefficients non-zero; z: n computed roots.
    Returns a dict: be[n] and r[n] (float64), gap, rel = max r/|z|, finite (all of z finite), n."""
    c = np.asarray(c, np.complex128).ravel()
    z = np.asarray(z, np.complex128).ravel()
    n = c.size - 1
    assert n >= 1 and z.size == n and c[0] != 0 and c[-1] != 0
    finite = bool(np.isfinite(z.real).all() and np.isfinite(z.imag).all())
    if not finite:
        return {"n": n, "finite": False, "be": np.full(n, np.inf), "r": np.full(n, np.inf), "gap": -np.inf, "rel": np.inf}
    zl = z.astype(CLD)
    inside = np.abs(z) <= 1.0
    absp = np.zeros(n, LD)        # |p| or |q|
    den = np.zeros(n, LD)
    logp = np.zeros(n, LD)        # log |p(z_k)|
    with np.errstate(divide="ignore"):
        if inside.any():
            p, s = _horner(c, zl[inside])
            absp[inside], den[inside] = np.abs(p), s
            logp[inside] = np.log(np.abs(p))
        if (~inside).any():
            x = CLD(1) / zl[~inside]
            q, s = _horner(c[::-1], x)
            absp[~inside], den[~inside] = np.abs(q), s
            logp[~inside] = np.log(np.abs(q)) + LD(n) * np.log(np.abs(zl[~inside]))
    be = (absp / den).astype(np.float64)
    # sum_{j != k} log |z_k - z_j|, rows in chunks
    rows = max(1, _CHUNK // n)
    lsum = np.zeros(n, np.float64)
    with np.errstate(divide="ignore"):
        for k0 in range(0, n, rows):
            k1 = min(n, k0 + rows)
            d = np.abs(z[k0:k1, None] - z[None, :])
            d[np.arange(k1 - k0), np.arange(k0, k1)] = 1.0
            lsum[k0:k1] = np.log(d).sum(axis=1)
        logr = np.log(LD(n)) + logp - np.log(LD(abs(c[0]))) - lsum.astype(LD)
        r = np.exp(logr).astype(np.float64)        # exp(-inf) = 0: p(z_k) = 0 exactly
    r = np.where(np.isnan(r), np.inf, r)           # coincident values: log 0 in the product
    gap = np.inf
    for k0 in range(0, n, rows):
        k1 = min(n, k0 + rows)
        g = np.abs(z[k0:k1, None] - z[None, :]) - r[k0:k1, None] - r[None, :]
        g[np.arange(k1 - k0), np.arange(k0, k1)] = np.inf
        gap = min(gap, float(g.min())) if n > 1 else gap
    if np.isnan(gap):
        gap = -np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = float(np.max(np.where(np.abs(z) > 0, r / np.abs(z), np.inf)))
    return {"n": n, "finite": True, "be": be, "r": r, "gap": gap, "rel": rel}


def be_bound(n):
    return 2.0 * n * U


def failures(cert):
    """The parts of the pass condition this certificate misses: a list of strings, empty when certified."""
    out = []
    if not cert["finite"]:
        out.append("not finite")
    if not cert["gap"] > 0.0:
        out.append("discs not disjoint (smallest gap %.3e)" % cert["gap"])
    if not np.max(cert["be"]) <= be_bound(cert["n"]):
        out.append("backward error %.3e n u > 2 n u" % (np.max(cert["be"]) / (cert["n"] * U)))
    return out


def figures(cert):
    """(max be / (n u), smallest gap, max r/|z|)"""
    return float(np.max(cert["be"]) / (cert["n"] * U)), cert["gap"], cert["rel"]


def certify(label, c, z):
    """Prints the figures of (c, z) and asserts the pass condition; returns the figures."""
    cert = certificate(c, z)
    f = figures(cert)
    print("%s: n %d  max be/(n u) %.4g  smallest gap %.4g  max r/|z| %.4g" % ((label, cert["n"]) + f))
    assert not failures(cert), (label, failures(cert))
    return f


# ---- polynomials with zero end coefficients ------------------------------------------------------------------------
def trim(c):
    """(nl, m, nt, c without its zero end coefficients): nl leading zeros are roots at infinity, nt trailing ones roots
    at zero, the root finders iterate on the m = n - nl - nt others."""
    c = np.asarray(c, np.complex128).ravel()
    nz = np.flatnonzero(c)
    nl, nt = int(nz[0]), int(c.size - 1 - nz[-1])
    return nl, c.size - 1 - nl - nt, nt, c[nl:c.size - nt]


def certify_with_ends(label, c, z):
    """z in the root finders' layout: the m finite non-zero roots, then nl at infinity, then nt zeros.  The certificate
    runs on the first m against the trimmed polynomial."""
    nl, m, nt, ct = trim(c)
    z = np.asarray(z).ravel()
    assert z.size == nl + m + nt
    assert np.isinf(z[m:m + nl].real).all() and (z[m + nl:] == 0).all(), label
    return certify(label, ct, z[:m])


def seg_len(m, S):
    """Powers per Newton segment of a sweep with S segments on degree m: ceil8(ceil((m + 1) / S))."""
    return ((m + 1 + S - 1) // S + 7) // 8 * 8


# ---- polynomial families (highest power first) ---------------------------------------------------------------------
def kac(n, seed):
    """Complex standard-normal coefficients: roots near the unit circle, well separated."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n + 1) + 1j * rng.standard_normal(n + 1)


def kac_scaled(n, seed, s):
    """kac(n, seed) with the coefficient of z^k multiplied by 2^(-s k), s = +1 or -1: exact in binary, so the roots are
    exactly the Kac roots times 2 (s = +1, all outside the unit circle) or 1/2 (s = -1, all inside)."""
    assert s in (1, -1) and n <= 513
    c = kac(n, seed)
    e = -s * (n - np.arange(n + 1))
    return np.ldexp(c.real, e) + 1j * np.ldexp(c.imag, e)


def two_scale(a, b, ra=0.4, rb=2.5):
    """(z^a - ra^a e^{0.3i}) (z^b - rb^b e^{1.1i}): a roots on |z| = ra and b on |z| = rb, so two hull slopes and roots
    on both sides of the unit circle; four non-zero coefficients (the rounded product is the polynomial certified)."""
    pa = np.zeros(a + 1, np.complex128)
    pb = np.zeros(b + 1, np.complex128)
    pa[0], pa[a] = 1.0, -(ra ** a) * np.exp(0.3j)
    pb[0], pb[b] = 1.0, -(rb ** b) * np.exp(1.1j)
    return np.convolve(pa, pb)


def zero_ends(nl, m, nt, c):
    """z^nt (z^m - c) with nl leading zero coefficients: degree nl + m + nt as stored."""
    p = np.zeros(nl + m + nt + 1, np.complex128)
    p[nl], p[nl + m] = 1.0, -c
    return p


def tm_blocks(polys):
    """polys[batch, n + 1] as entry 11 of 4*(n + 1) transfer-matrix blocks, the layout NftDiscSpecSearch::roots reads."""
    polys = np.asarray(polys, np.complex128)
    tm = np.zeros((polys.shape[0], 4, polys.shape[1]), np.complex128)
    tm[:, 0, :] = polys
    return tm
