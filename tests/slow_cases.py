"""Cases shared by the slow-discretization tests (emulator and GPU): signals, the xi-grid, the extended-precision
reference (tests/slow_ref.py) computed once per case, and the error metric of the accuracy bound."""
import functools

import numpy as np

import signals as S
import slow_ref as SR

DISCS = SR.DISCS
T_FOC, T_DEF = (-10.0, 10.0), (-2.0, 1.5)
XI = (-1.4, 1.6)
MARGIN = 4.0     # e <= MARGIN * e_dbl: room for rounding order, 1-2 ulp device functions and another FFT


def interval(kappa):
    return T_FOC if kappa == 1 else T_DEF


def signal(D, kappa, variant=0):
    """sech_focusing / sech_defocusing times a linear phase, so that q is not real; `variant` changes amplitude and phase
    slope (the signals of a batch differ)."""
    T = interval(kappa)
    t = S.tgrid(T, D)
    if kappa == 1:
        q = S.sech_focusing(D, T=T, amp=3.2 - 0.35 * variant)
    else:
        q = S.sech_defocusing(D, T=T) * (1.0 - 0.1 * variant)
    return (q * np.exp(1j * (0.3 + 0.2 * variant) * t)).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def reference(disc, kappa, D, M, richardson=0, variant=0):
    """(long-double spectrum, e_dbl): dicts by 'rho', 'a', 'b'; e_dbl is the error of the same code run in double."""
    q = signal(D, kappa, variant)
    T = interval(kappa)
    ld = SR.nsev_slow(q, T, M, XI, kappa, disc, richardson)
    db = SR.nsev_slow(q, T, M, XI, kappa, disc, richardson, dtype=np.complex128)
    return ld, {k: SR.rel_max(db[k], ld[k]) for k in ld}


def split_both(out, M):
    """contspec_type BOTH of one signal -> dict."""
    out = np.asarray(out).reshape(-1)
    return {"rho": out[:M], "a": out[M:2 * M], "b": out[2 * M:3 * M]}


def check(tag, got, disc, kappa, D, M, richardson=0, variant=0):
    """Prints e and e_dbl of rho, a, b, then asserts e <= MARGIN * e_dbl for each; returns the figures."""
    ld, e_dbl = reference(disc, kappa, D, M, richardson, variant)
    e = {k: SR.rel_max(got[k], ld[k]) for k in ld}
    print("%s %s kappa=%+d D=%d M=%d rich=%d: " % (tag, disc, kappa, D, M, richardson)
          + "  ".join("%s e=%.2e e_dbl=%.2e" % (k, e[k], e_dbl[k]) for k in ("rho", "a", "b")))
    for k in ("rho", "a", "b"):
        assert e[k] <= MARGIN * e_dbl[k], (tag, disc, kappa, D, M, k, e[k], e_dbl[k])
    return e, e_dbl
