"""Extended-precision reference for the chirp z-transform and its epilogues (helper module, not a test).

Chirp z-values: X_m = sum_n c_n A^-n W^(n m), c_n = p[deg - n] (fnft__poly_chirpz), evaluated at K chosen output
indices m in np.clongdouble (64-bit significand), chunked over n so that memory stays bounded at deg ~ 2^24.  A and W
are the doubles the product receives; log A and log W are formed from them exactly (mpmath) and rounded to long double
once, so |A| and |W| that are 1 only up to rounding act as they do in the kernels (which take nft_clog of the same
doubles).  In DFT mode (A = 1, W = exp(+-2 pi i / len)) every power comes from the exact integer residue (n m) mod len,
as the kernels form their chirp: that path carries no phase error at all.

Metric: e = max over the K points of |X_gpu - X_ref| / mass, mass = sum |c_n| |A|^-n: a correct transform of length L
is good to about u log2 L relative to that mass, plus the rounding of the chirp phases n^2 arg(W)/2 + n arg(A) that
the kernels (and the reference algorithm) form in double -- an inherent error of u Phi, Phi the largest such phase.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
CLD = np.clongdouble
_PI = LD("3.141592653589793238462643383279502884197169399375105820974944592307816406286208998628034825342117068")
_TAU = 2 * _PI
_CHUNK = 1 << 18     # coefficients per evaluation chunk (x K points x 32 bytes)
_SPLIT = 13          # exact residues r < 2^26 as r_hi 2^13 + r_lo: two table look-ups and one long-double product


def ld(x):
    """An mpmath number (or anything str() renders exactly enough) -> np.longdouble."""
    import mpmath
    return LD(mpmath.nstr(x, 30, strip_zeros=False)) if isinstance(x, mpmath.mpf) else LD(x)


def ld_log(z):
    """log of the complex double z, formed exactly and rounded to long double: (re, im)."""
    import mpmath
    with mpmath.workprec(160):
        w = mpmath.log(mpmath.mpc(float(np.real(z)), float(np.imag(z))))
        return ld(w.real), ld(w.imag)


def unit_pow(r, N):
    """exp(2 pi i r / N) for integers 0 <= r < N (int64 array, N < 2^26) in clongdouble, from two small tables."""
    r = np.asarray(r, np.int64)
    nlo = 1 << _SPLIT
    nhi = (N + nlo - 1) // nlo
    a_lo = np.arange(nlo, dtype=LD) * (_TAU / LD(N))
    a_hi = (np.arange(nhi, dtype=np.int64) * nlo).astype(LD) * (_TAU / LD(N))
    t_lo = (np.cos(a_lo) + 1j * np.sin(a_lo)).astype(CLD)
    t_hi = (np.cos(a_hi) + 1j * np.sin(a_hi)).astype(CLD)
    return t_hi[r >> _SPLIT] * t_lo[r & (nlo - 1)]


def chirpz_ref(p, A, W, m, dft=None):
    """X_m = sum_n p[deg-n] A^-n W^(n m) at the output indices m (int array): (values (K,) clongdouble, mass).
    dft = (len, sign): DFT mode, A = 1 and W = exp(sign 2 pi i / len), p in ascending order (x[n] multiplies z^n, the
    layout of the kernels' DFT mode), every power from the residue (n m) mod len."""
    p = np.asarray(p)
    m = np.asarray(m, np.int64)
    out = np.zeros(m.size, CLD)
    if dft is not None:
        ln, sg = dft
        c = p
        for j0 in range(0, c.size, _CHUNK):
            n = np.arange(j0, min(c.size, j0 + _CHUNK), dtype=np.int64)
            r = (n[None, :] * m[:, None]) % ln
            if sg < 0:
                r = (ln - r) % ln
            out += np.sum(c[j0:j0 + n.size].astype(CLD)[None, :] * unit_pow(r, ln), axis=1)
        return out, LD(np.sum(np.abs(c.astype(CLD))))
    la, lw = ld_log(A), ld_log(W)    # (re, im) pairs
    c = p[::-1]
    mass = LD(0)
    for j0 in range(0, c.size, _CHUNK):
        n = np.arange(j0, min(c.size, j0 + _CHUNK), dtype=np.int64)
        nl = n.astype(LD)
        nm = (n[None, :] * m[:, None]).astype(LD)      # exact: n m < 2^64
        re = -nl[None, :] * la[0] + nm * lw[0]
        im = -nl[None, :] * la[1] + nm * lw[1]
        pw = np.exp(re + CLD(1j) * im)
        cc = c[j0:j0 + n.size].astype(CLD)
        out += np.sum(cc[None, :] * pw, axis=1)
        mass += np.sum(np.abs(cc) * np.exp(-nl * la[0]))
    return out, mass


def phi(L, A, W):
    """Phi = max over n < L of n^2 |arg W| / 2 + n |arg A|: the largest chirp phase the kernels round in double."""
    la, lw = ld_log(A), ld_log(W)
    n = float(L - 1)
    return n * n * abs(float(lw[1])) / 2.0 + n * abs(float(la[1]))


def err_bound(C, L, Phi=0.0):
    """u (A log2 L + P Phi) with C = (A, P): L the chirp transform length, Phi the largest chirp (and epilogue) phase
    rounded in double (0 in DFT mode)."""
    A, P = C
    return U * (A * np.log2(L) + P * Phi)


def error(x, ref, mass):
    """e = max |x - ref| / mass over the K points (x: the product's values there)."""
    return float(np.max(np.abs(np.asarray(x).astype(CLD) - ref)) / mass)


# ---- fnft__misc_resample in closed form --------------------------------------------------------------------------
def resample_ref(q, eps_t, delta, j):
    """q_new[j] = sum_n q_n h(j - n) at the output indices j, h(d) = (1/D) sum_f exp(i f phi_d),
    phi_d = 2 pi (delta/(D eps_t) + d/D), f over the reference's frequency grid f = k (k < D/2), k - D (k >= D/2)
    (fnft__misc.c:383-393; body_resample_phase).  The geometric sum is
        sum_{f=f0}^{f0+D-1} e^(i f phi) = e^(i phi (f0 + (D-1)/2)) sin(D phi/2) / sin(phi/2),
    f0 + (D-1)/2 = -1 (D odd) or -1/2 (D even), sin(D phi_d/2) = (-1)^d sin(pi x), x = delta/eps_t; the phi -> 0 limit
    is D.  O(D) per output point."""
    q = np.asarray(q).astype(CLD)
    D = q.size
    x = LD(delta) / LD(eps_t)
    xi = int(np.round(x))
    xr = x - LD(xi)                                          # exact: x = xi + xr, |xr| <= 1/2
    sx = (-1) ** (xi % 2) * np.sin(_PI * xr)                 # sin(pi x) without the cancellation near integers
    ex = np.cos(_PI * x / D) + 1j * np.sin(_PI * x / D)      # e^(i pi x / D)
    n = np.arange(D, dtype=np.int64)
    out = np.zeros(len(j), CLD)
    for k, jj in enumerate(np.asarray(j, np.int64)):
        d = jj - n
        e = unit_pow(d % (2 * D), 2 * D) * CLD(ex)           # e^(i phi_d / 2), residues exact
        s = e.imag.astype(LD)
        # near phi = 0 (mod 2 pi) the table product's absolute error (~1e-19) would be a large relative error of
        # sin(phi/2): take the sine directly there, sin(y + k pi) = (-1)^k sin(y)
        kk = np.round((d + xi) / D).astype(np.int64)        # nearest multiple of 2 pi
        y = xr + (d + xi - kk * D).astype(LD)
        near = np.abs(y) < 4096
        s[near] = np.where(kk[near] % 2 == 0, LD(1), LD(-1)) * np.sin(_PI * y[near] / D)
        ph = np.conj(e) ** 2 if D % 2 else np.conj(e)        # e^(i phi (f0 + (D-1)/2))
        sgn = np.where(d % 2 == 0, LD(1), LD(-1))
        zero = s == 0
        h = ph * (sgn * sx) / (LD(D) * np.where(zero, LD(1), s))
        h[zero] = 1
        out[k] = np.sum(q * h)
    return out


def resample_mass(q):
    """Scale of the resampler's error: the rms of the samples (the per-point error of a DFT -> ramp -> inverse DFT
    of length-L chirps is about u log2 L times it)."""
    q = np.asarray(q)
    return float(np.sqrt(np.mean(np.abs(q) ** 2)))


# ---- epilogues ---------------------------------------------------------------------------------------------------
def nsev_grid(T, XI, M, Dg, deg1):
    """The chirp points of run_contspec_impl (fnft_nsev.c:822-827): (A, V) as the doubles the host forms, and the
    long-double xi_m = XI0 + m eps_xi and eps_t.  deg1 = degree per kept step times upsampling, Dg = given samples."""
    import math
    eps_t = (T[1] - T[0]) / float(Dg - 1)
    eps_xi = (XI[1] - XI[0]) / float(M - 1)
    phiV = 2.0 * eps_xi * eps_t / float(deg1)
    phiA = 2.0 * (-XI[0]) * eps_t / float(deg1)
    return complex(math.cos(phiA), math.sin(phiA)), complex(math.cos(phiV), math.sin(phiV))


def kdvv_grid(T, XI, M, D, deg1):
    """The chirp points of run_contspec_kdv (fnft_kdvv.c:159-160)."""
    import math
    eps_t = (T[1] - T[0]) / float(D - 1)
    eps_xi = (XI[1] - XI[0]) / float(M - 1)
    phiV = -2.0 * eps_xi * eps_t / float(deg1)
    phiA = 2.0 * XI[0] * eps_t / float(deg1)
    return complex(math.cos(phiA), math.sin(phiA)), complex(math.cos(phiV), math.sin(phiV))


def _cis(a):
    return (np.cos(a) + 1j * np.sin(a)).astype(CLD)


def nsev_phase_factors(T, XI, M, Dg, deg1, shifted, m):
    """xi_m and the phase factors of fnft_nsev.c:837-884 (boundary coefficient 0.5) in long double."""
    T0, T1 = LD(T[0]), LD(T[1])
    eps_t = (T1 - T0) / LD(Dg - 1)
    xi = LD(XI[0]) + (LD(XI[1]) - LD(XI[0])) / LD(M - 1) * np.asarray(m).astype(LD)
    sh = eps_t / LD(deg1) if shifted else LD(0)
    pf_rho = -2 * (T1 + eps_t / 2) + sh
    pf_a = -eps_t * LD(Dg) + (T1 + eps_t / 2) - (T0 - eps_t / 2)
    pf_b = -eps_t * LD(Dg) - (T1 + eps_t / 2) - (T0 - eps_t / 2) + sh
    return xi, pf_rho, pf_a, pf_b


def nsev_epilogue_ref(tm, W, T, XI, M, Dg, deg1, shifted, m):
    """rho, a, b (fnft_nsev.c:837-884) at the output indices m from the transfer matrix tm [4, deg+1] (true matrix
    tm * 2^W), and the masses: dict(rho, a, b, H11, mass, phi_pf)."""
    A, V = nsev_grid(T, XI, M, Dg, deg1)
    H11, m11 = chirpz_ref(tm[0], A, V, m)
    H21, m21 = chirpz_ref(tm[2], A, V, m)
    xi, pf_rho, pf_a, pf_b = nsev_phase_factors(T, XI, M, Dg, deg1, shifted, m)
    s = np.ldexp(LD(1), int(W))
    return dict(rho=H21 / H11 * _cis(xi * pf_rho), a=H11 * s * _cis(xi * pf_a), b=H21 * s * _cis(xi * pf_b),
                H11=H11, mass=max(m11, m21), scale=s,
                phi_pf=float(np.max(np.abs(xi)) * max(abs(pf_rho), abs(pf_a), abs(pf_b))))


def kdvv_epilogue_ref(tm, T, XI, M, D, deg1, scheme_2A, m):
    """The KdV reflection coefficient (fnft_kdvv.c:186-203) at the output indices m: dict(rho, den, mass, phi_pf)."""
    A, V = kdvv_grid(T, XI, M, D, deg1)
    H12, m12 = chirpz_ref(tm[1], A, V, m)
    H22, m22 = chirpz_ref(tm[3], A, V, m)
    T0, T1 = LD(T[0]), LD(T[1])
    eps_t = (T1 - T0) / LD(D - 1)
    xi = -(LD(XI[0]) + (LD(XI[1]) - LD(XI[0])) / LD(M - 1) * np.asarray(m).astype(LD))
    pf_rho = 2 * (T1 + eps_t / 2)
    pf_a = -eps_t / LD(deg1) if scheme_2A else LD(0)
    H12 = H12 * _cis(xi * pf_a)          # the 2SPLIT2A correction comes first: numerator and denominator see it
    den = 2j * xi * H22 - H12
    xmax = np.max(np.abs(xi))
    return dict(rho=H12 * _cis(xi * pf_rho) / den, den=den, mass=m12 + 2 * xmax * m22,
                phi_pf=float(xmax * (abs(pf_rho) + abs(pf_a))))


def quotient_error(x, ref, den, mass):
    """First-order error of a quotient: max |x - ref| |den| / mass (a tiny denominator does not widen the bound)."""
    d = np.abs(np.asarray(x).astype(CLD) - ref) * np.abs(den)
    return float(np.max(d) / mass)
