"""Extended-precision reference for the polynomial-matrix product tree (helper module, not a test).

A transfer matrix T(z) = P_0(z) P_1(z) ... P_{n-1}(z) is compared with what the tree returned at a few points
z_k = exp(2 pi i m_k / P) of the unit circle, P a prime (no transform length 2^a or 3*2^a is a multiple of it, so
no z_k is a root of unity of any length the kernels use).  Every power z^j is looked up as exp(2 pi i ((j m_k) mod P)
/ P) in a table of long-double sines: no repeated multiplication, so the points carry no error that grows with the
degree.  Sums run in np.clongdouble (64-bit significand: 2^11 times finer than the fp64 error being measured).

Metric: e = max over points and entries of |T_gpu(z_k) - T_ref(z_k)| / mass, mass = sum |c| over the coefficients c
of all four entries (both sides in the same power-of-two scale).  A correct FFT product of length N is accurate to
about u log2 N relative to that mass, u = 2^-53.
"""
import numpy as np

U = 2.0 ** -53
PRIME = 1000003
LD = np.longdouble
CLD = np.clongdouble
_TAU = LD("6.283185307179586476925286766559005768394338798750211641949889184615632812572417997256069650684234136")
_CHUNK = 1 << 18   # coefficients per evaluation chunk (x K points x 32 bytes)
_table = None


def unit_table():
    """exp(2 pi i r / PRIME), r = 0 .. PRIME-1, in clongdouble (computed once per process)."""
    global _table
    if _table is None:
        a = np.arange(PRIME, dtype=LD) * (_TAU / LD(PRIME))
        _table = (np.cos(a) + 1j * np.sin(a)).astype(CLD)
    return _table


def points(K, salt=0):
    """K distinct exponents m_k in (0, PRIME), spread over the circle (deterministic)."""
    rng = np.random.default_rng(7919 + 31 * K + salt)
    base = (np.arange(K) + rng.uniform(0.1, 0.9, K)) / K
    m = np.unique(np.clip(np.round(base * PRIME).astype(np.int64), 1, PRIME - 1))
    assert m.size == K
    return m


def powers(exps, m):
    """z_k^e for every exponent e (int64 array) and point m_k: shape (K, len(exps))."""
    T = unit_table()
    return T[(np.asarray(exps, np.int64)[None, :] * np.asarray(m, np.int64)[:, None]) % PRIME]


def eval_polys(c, m):
    """c: (rows, L) coefficients, highest power first (the reference layout).  Values at the points m: (rows, K)
    clongdouble.  Chunked over the coefficients and rows so that memory stays bounded at any degree."""
    c = np.asarray(c)
    rows, L = c.shape
    out = np.zeros((rows, len(m)), CLD)
    rchunk = max(1, _CHUNK // max(L, 1))
    for j0 in range(0, L, _CHUNK):
        j1 = min(L, j0 + _CHUNK)
        pw = powers(L - 1 - np.arange(j0, j1), m).T          # (j1-j0, K)
        for r0 in range(0, rows, rchunk):
            r1 = min(rows, r0 + rchunk)
            out[r0:r1] += np.matmul(c[r0:r1, j0:j1].astype(CLD), pw)
    return out


def eval_result(res, m):
    """Result in the reference layout [4, deg+1] -> values (K, 2, 2) and mass = sum |c| (both unscaled)."""
    v = eval_polys(res, m)                                   # (4, K)
    mass = LD(np.sum(np.abs(res)))
    return np.moveaxis(v, 0, 1).reshape(len(m), 2, 2), mass


def factor_values(p, deg, n, m):
    """p: [4, n*(deg+1)] factor coefficients (reference layout) -> values (n, K, 2, 2) clongdouble."""
    p = np.asarray(p).reshape(4 * n, deg + 1)
    v = eval_polys(p, m).reshape(4, n, len(m))
    return np.moveaxis(v, 0, -1).reshape(n, len(m), 2, 2)


def _renorm(F, E):
    """F * 2^E with every matrix's largest entry brought into [0.5, 1) (E: int64 per matrix)."""
    mx = np.max(np.abs(F), axis=(-2, -1))
    _, e = np.frexp(np.where(mx > 0, mx, LD(1)))
    return F * np.ldexp(LD(1), -e)[..., None, None], E + e


def ordered_product(F):
    """Ordered product F_0 F_1 ... F_{n-1} of (n, K, 2, 2) matrices, balanced pairwise reduction with a power-of-two
    exponent per matrix (the products of scaled factors leave the long-double range).  Returns (values (K, 2, 2),
    exp2 (K,)): the product is values * 2^exp2."""
    F, E = _renorm(np.asarray(F, CLD), np.zeros(np.shape(F)[:2], np.int64))
    lvl = 0
    while F.shape[0] > 1:
        h = F.shape[0] // 2 * 2
        G, Eg = np.matmul(F[0:h:2], F[1:h:2]), E[0:h:2] + E[1:h:2]
        lvl += 1
        if lvl % 8 == 0 or h <= 2:   # entries grow by at most 2x per level in between
            G, Eg = _renorm(G, Eg)
        F, E = (np.concatenate([G, F[h:]]), np.concatenate([Eg, E[h:]])) if h < F.shape[0] else (G, Eg)
    return F[0], E[0]


def tree_ref(p, deg, n, m, exp2=0):
    """Exact product of the n factors p * 2^exp2 (p: [4, n*(deg+1)]) at the points m: (values (K, 2, 2), exp2 (K,))."""
    v, e = ordered_product(factor_values(p, deg, n, m))
    return v, e + int(exp2) * n


def error(res, W, ref, m):
    """e = max |T_gpu - T_ref| / mass.  res, W: the tree's result (true matrix res * 2^W); ref = (values, exp2) of
    tree_ref at the points m."""
    vals, e2 = ref
    v, mass = eval_result(res, m)
    # both sides in the scale of the result: T_ref * 2^-W
    r = vals * np.ldexp(LD(1), (np.asarray(e2, np.int64) - int(W)))[:, None, None]
    return float(np.max(np.abs(v - r)) / mass)


def err_bound(C, N, n=0):
    """u (A log2 N + B n) with C = (A, B): N the longest transform of the tree, n the number of factors.  The top product
    alone is good to about u log2 N; the products of the lower levels add errors of a fixed relative size per factor,
    which reach the root scaled by the rest of the product (the double-precision FFT tree of the oracle shows
    e = 0.2 u n for a sech-pulse signal from 2^10 to 2^16 samples, with identical factors).  So on a tree of many
    factors the n term dominates, and one upper-level kernel a few hundred times worse than its own u log2 N would not
    be seen there: the cases with few factors of a high degree are the ones that pin a kernel at its own accuracy."""
    A, B = C
    return U * (A * np.log2(N) + B * n)
