"""Inputs of the batched discrete-spectrum tests (test_discspec_batch_emu.py, test_gpu_nsev_batch_discrete.py):
chirped sech pulses q(t) = i A sech(t) exp(i c t) on T = [-25, 25], whose eigenvalues are -c/2 + i (A - 1/2 - k),
and Newton start values around them."""
import numpy as np

import signals as S

T = (-25.0, 25.0)
PAIRS = [(1.2, 0.0), (1.7, 0.4), (2.2, -0.6), (2.7, 1.0), (3.2, 0.4), (3.7, -0.3), (2.4, 0.8), (1.9, -1.2)]
K_OUT = [1, 2, 2, 3, 3, 4, 2, 2]     # bound states of the eight pulses
OFFSET_2SPLIT = 0.07 - 0.05j
DUP_2SPLIT = -0.05 + 0.04j            # a second guess near the first eigenvalue: merged away
OFFSET_4SPLIT = 0.01 + 0.01j          # CF4_2 Newton wanders from the larger offset; no duplicate guess


def signal(D, A, c):
    return (S.sech_focusing(D, T, amp=A) * np.exp(1j * c * S.tgrid(T, D))).astype(np.complex128)


def exact_eigenvalues(A, c):
    k = np.arange(int(np.ceil(A - 0.5)))
    return -0.5 * c + 1j * (A - 0.5 - k)


def guesses(A, c, K, offset, dup=None):
    """K start values: the eigenvalues + offset, optionally one more near the first eigenvalue, the rest below the
    real axis (filtered by BASIC and FULL)."""
    g = list(exact_eigenvalues(A, c) + offset)
    if dup is not None and len(g) < K:
        g.append(exact_eigenvalues(A, c)[0] + dup)
    g = g[:K]
    g += [-0.5 * c - 0.4j] * (K - len(g))
    return np.array(g, np.complex128)


def batch(D, K, four_split, pairs=PAIRS):
    off, dup = (OFFSET_4SPLIT, None) if four_split else (OFFSET_2SPLIT, DUP_2SPLIT)
    q = np.stack([signal(D, A, c) for A, c in pairs])
    g = np.stack([guesses(A, c, K, off, dup) for A, c in pairs])
    return q, g


_ORACLE = {}


def oracle_reference(oracle, disc, D, K, pairs=PAIRS):
    """Per signal (rc, bound states, norming constants, residues, |a| at the bound states) of the oracle with NEWTON,
    FULL filtering, niter = 10; computed once per (disc, D, K, pairs)."""
    key = (disc, D, K, tuple(pairs))
    if key not in _ORACLE:
        four = disc.startswith("4SPLIT")
        q, g = batch(D, K, four, pairs)
        eps_t = (T[1] - T[0]) / (D - 1)
        out = []
        for b in range(len(pairs)):
            rc, bs, nc, res = oracle.fnft_nsev_ds(q[b], T, disc, bsloc="NEWTON", bsfilt="FULL", niter=10, guesses=g[b])
            a = None
            if rc == 0 and bs.size:
                _, qp, _, _ = oracle.preprocess(q[b], eps_t, D, disc)
                _, a, _, _ = oracle.scatter_bound_states(qp, T, bs, 2 if four else 1, skip_b=True)
            out.append((rc, bs, nc, res, None if a is None else np.abs(a)))
        _ORACLE[key] = out
    return _ORACLE[key]

