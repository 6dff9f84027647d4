"""Plain sequential layer peeling: the reference of the peeling path tests (tests/test_peel_cases_cpu.py,
tests/test_gpu_peel_paths.py).

A restatement of the base case of src/private/fnft__nse_finvscatter.c:158-196 applied d times, without the
recursion: the last step matrix scl [[1, Q z], [-kappa Q*, z]] is divided out of the first column of the transfer
matrix, one sample per step,
    Q = -kappa conj(T21(0) / T11(0)),        T11 <- T11 - Q T21,        T21 <- (kappa Q* T11 + T21) / z
(both updates from the arrays before the step; without the factor scl, which Q, a ratio, never sees).  The second
column of T does not influence the samples.  In numpy.clongdouble the result is the answer to the question the
kernels are asked -- the same double-precision tm [4, d + 1] goes in -- with an error of about 1e-19 times the
conditioning; in complex128 the same code is one of the two yardsticks of the GPU bound.
"""
import numpy as np

U = 2.0 ** -53
_REAL = {np.clongdouble: np.longdouble, np.complex128: np.float64}


def peel_steps(tm, kappa, ctype=np.clongdouble, q_factor=None, kappa_t21=None):
    """tm [4, d+1] (highest power first) -> (rc, Q[d]) in arithmetic of type ctype: Q[n] is the step parameter of
    sample n (the last sample is peeled first).  rc = 5 if a step has 1 + kappa |Q|^2 <= 0 (:173-176).
    q_factor, kappa_t21: deliberately wrong variants for the sensitivity check -- every Q times q_factor; another
    kappa in the update of T21 only."""
    rt = _REAL[ctype]
    tm = np.asarray(tm)
    t1, t2 = tm[0].astype(ctype), tm[2].astype(ctype)
    d = t1.size - 1
    k = rt(kappa)
    k2 = k if kappa_t21 is None else rt(kappa_t21)
    Qs = np.zeros(d, ctype)
    for s in range(d):                       # coefficients s .. d are left; index d is the constant term
        Q = -k * np.conj(t2[d] / t1[d])
        if q_factor is not None:
            Q = Q * rt(q_factor)
        if not 1 + k * (Q.real * Q.real + Q.imag * Q.imag) > 0:
            return 5, None
        Qs[d - 1 - s] = Q
        n1 = t1[s:] - Q * t2[s:]
        n2 = k2 * np.conj(Q) * t1[s:d] + t2[s:d]
        t1[s:] = n1
        t2[s + 1:] = n2                      # division by z
        t2[s] = 0
    return 0, Qs


def samples(Q, eps_t, disc):
    """Step parameters -> samples, in the type of Q: Q / eps_t (2SPLIT2_MODAL, :190) or atan|Q| e^{i arg Q} / eps_t
    (2SPLIT2A, :210)."""
    Q = np.asarray(Q)
    e = _REAL[Q.dtype.type](eps_t)
    if disc == "2SPLIT2_MODAL":
        return Q / e
    assert disc == "2SPLIT2A", disc
    a = np.abs(Q)
    safe = np.where(a > 0, a, 1)
    return np.where(a > 0, np.arctan(a) / safe, 1) * Q / e


def peel(tm, eps_t, kappa, disc, ctype=np.clongdouble, **wrong):
    """tm [4, d+1] -> (rc, q[d]): the samples of fnft__nse_finvscatter by d sequential steps in ctype."""
    rc, Q = peel_steps(tm, kappa, ctype, **wrong)
    return rc, (samples(Q, eps_t, disc) if rc == 0 else None)


def error(q, q_ref):
    """max |q - q_ref| / max |q_ref| (in the wider of the two types)."""
    q_ref = np.asarray(q_ref)
    return float(np.max(np.abs(np.asarray(q) - q_ref)) / np.max(np.abs(q_ref)))
