"""Shapes, points and signals of the polynomial evaluation tests (tests/test_polyeval_emu.py in the CPU lane emulator,
tests/test_gpu_polyeval.py on the GPU).  Helper module, not a test; everything is deterministic.

TILE is kPolyEvalTile (nft_dispatch.h), the coefficients a workgroup stages per tile; 8 is the chain count; a workgroup
takes 256 points.  The shapes put a degree on either side of each: 7 | 8 | 9 chains, TILE-1 | TILE | TILE+1 and
2 TILE + 5 tiles, 63 | 64 | 65 a wave, 257 a second workgroup."""
import zlib

import numpy as np

TILE = 512
DEGS = (0, 1, 3, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)
NZS = (1, 63, 64, 65, 257)
DEG0 = {"2SPLIT2_MODAL": 1, "2SPLIT2A": 1, "2SPLIT4B": 2, "4SPLIT4A": 4, "4SPLIT4B": 2}
UPS = {"2SPLIT2_MODAL": 1, "2SPLIT2A": 1, "2SPLIT4B": 1, "4SPLIT4A": 2, "4SPLIT4B": 2}


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def coefficients(shape, *key):
    r = rng("c", *key)
    return r.standard_normal(shape) + 1j * r.standard_normal(shape)


def points(nz, *key, rmax=1.5):
    """nz points that mix, inside every wave, the regimes of src/private/fnft__poly_eval.c: |z| < 1, exp(i theta) as
    libm rounds it (|z|^2 = 1 -+ u: either branch), |z| = 1 -+ 1e-9 (the reciprocal matters most there), 1 < |z| <= rmax,
    and -- from 8 points on -- |z| = 1 exactly (1, -1, i, -i) and z = 0."""
    r = rng("z", nz, *key)
    kind = r.permutation(np.arange(nz) % 4)
    th = r.uniform(0.0, 2.0 * np.pi, nz)
    rad = np.where(kind == 0, np.sqrt(r.uniform(0.0, 1.0, nz)),
                   np.where(kind == 1, 1.0, np.where(kind == 2, 1.0 + r.choice([-1e-9, 1e-9], nz),
                                                     r.uniform(1.0, rmax, nz))))
    z = rad * np.exp(1j * th)
    if nz >= 8:
        at = (np.arange(5) * nz) // 5 + 1
        z[at] = [1.0, -1.0, 1j, -1j, 0.0]
    return z


def lambdas(n, T, kind, *key):
    """n points: "real" in [-3, 3]; "complex": Im of both signs with |Im lambda| (T1 - T0) <= 8."""
    r = rng("l", n, kind, *key)
    re = r.uniform(-3.0, 3.0, n)
    if kind == "real":
        return re.astype(np.complex128)
    im = r.uniform(-1.0, 1.0, n) * 8.0 / (T[1] - T[0])
    im[: min(2, n)] = np.array([8.0, -8.0])[: min(2, n)] / (T[1] - T[0])
    return re + 1j * im


def nse_signal(D, T, batch, *key):
    """`batch` signals of D samples: a complex pulse of amplitude about one, another per signal."""
    r = rng("q", D, batch, *key)
    t = np.linspace(T[0], T[1], D)
    out = []
    for b in range(batch):
        a, w, c = r.uniform(0.6, 1.4), r.uniform(0.5, 1.5), r.uniform(-0.5, 0.5)
        out.append(a / np.cosh(w * (t - c)) * np.exp(1j * (r.uniform(-1, 1) * t + 0.3 * b))
                   + 0.05 * (r.standard_normal(D) + 1j * r.standard_normal(D)))
    return np.array(out)
