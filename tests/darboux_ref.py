"""The discrete part of fnft_nsev_inverse in extended precision: the reference of the Darboux path tests
(tests/test_darboux_cases_cpu.py, tests/test_darboux_emu.py, tests/test_gpu_darboux_paths.py).

A restatement of src/fnft_nsev_inverse.c:680-1007 in numpy.clongdouble, starting from the same doubles the kernels get
(bound states, norming constants or residues, seed samples, T, D): the exchange sort (:742-754), the conversion of
residues with a = 1 (:771-795), the multi-soliton recursion (:797-842), the half-step exponential integrator of the
eigenfunctions (:908-1007) and the Darboux steps (:864-889).  The step eps_t = (T1 - T0)/(D - 1) is formed in double, as
the host forms it; the grid t_n = T0 + eps_t n in long double.  Every function takes the complex type, so the same code in
complex128 serves as a yardstick.

One deliberate difference from the reference: where ks = q r - lambda^2 is exactly 0 the reference skips the half step
(:941-948, 955, 980, 995); here, as in the kernels' shared step function (bs_step_r), the step is the limit
sinh(k h)/k -> h.  skip_ks_zero=True restates the reference.

cdt_exact_zero_seed_ref is a second algorithm for the pure multi-soliton: Darboux steps on the zero potential with its
exact eigenfunctions.  It shares nothing with the recursion of solitons_ref but the inputs.
"""
import numpy as np

U = 2.0 ** -53
_REAL = {np.clongdouble: np.longdouble, np.complex128: np.float64}


def error(q, q_ref):
    """max |q - q_ref| / max |q_ref| (in the wider of the two types)."""
    q_ref = np.asarray(q_ref)
    return float(np.max(np.abs(np.asarray(q) - q_ref)) / np.max(np.abs(q_ref)))


def sort_bound_states(bs, nc):
    """The reference's exchange sort by descending imaginary part (:742-754), on copies, in the type given."""
    bs, nc = np.array(bs), np.array(nc)
    K = bs.size
    for i in range(K):
        for j in range(i + 1, K):
            if bs[i].imag < bs[j].imag:
                bs[i], bs[j] = bs[j], bs[i]
                nc[i], nc[j] = nc[j], nc[i]
    return bs, nc


def residues_to_normconsts_ref(bs, res, ctype=np.clongdouble):
    """:771-795 with a(lambda_k) = 1: sorted bound states and residues -> norming constants."""
    bs, res = np.asarray(bs).astype(ctype), np.asarray(res).astype(ctype)
    K = bs.size
    nc = np.zeros(K, ctype)
    for i in range(K):
        tmp = ctype(1)
        for j in range(K):
            if j != i:
                tmp = tmp * (bs[i] - bs[j]) / (bs[i] - np.conj(bs[j]))
        nc[i] = (res[i] / (ctype(2j) * bs[i].imag)) * tmp
    return nc


def prepared(bs, nc_or_res, residues, ctype=np.clongdouble):
    """Sorted bound states and norming constants in ctype, from the caller's doubles."""
    b, c = sort_bound_states(np.asarray(bs, np.complex128), np.asarray(nc_or_res, np.complex128))
    b, c = b.astype(ctype), c.astype(ctype)
    if residues:
        c = residues_to_normconsts_ref(b, c, ctype)
    return b, c


def grid(T, D, ctype=np.clongdouble):
    """(eps_t in double, t_n = T0 + eps_t n in the real type of ctype, zc as the host computes it: the first n with
    T0 + eps_t n >= 0 in double, 0 if there is none)."""
    rt = _REAL[ctype]
    eps_t = (float(T[1]) - float(T[0])) / (D - 1)
    t = rt(T[0]) + rt(eps_t) * np.arange(D).astype(rt)
    td = float(T[0]) + eps_t * np.arange(D, dtype=np.float64)
    zc = int(np.argmax(td >= 0.0)) if np.any(td >= 0.0) else 0
    return eps_t, t, zc


# ---- pure solitons, :797-842 -----------------------------------------------------------------------------------------
def _recursion(bs, rhok, ctype):
    K = bs.size
    qt = np.zeros(rhok.shape[1], ctype)
    for i in range(K):
        rho = rhok[i].copy()
        rhoc = np.conj(rho)
        f = (ctype(2j) * bs[i].imag) / (1 + rho.real * rho.real + rho.imag * rho.imag)
        qt = qt + ctype(2j) * rhoc * f
        for j in range(i + 1, K):
            rhok[j] = ((bs[j] - bs[i]) * rhok[j] + (rhok[j] - rho) * f) / (
                bs[j] - np.conj(bs[i]) - (1 + rhoc * rhok[j]) * f)
    return qt


def solitons_ref(bs, nc, T, D, ctype=np.clongdouble, t=None):
    """bs, nc: prepared().  rho_k = b_k exp(2 i lambda_k t) and the recursion on the samples n >= zc; the mirrored
    recursion (1/b_k, -t, conjugate) on those before.  t: another grid in place of T0 + eps_t n (yardsticks)."""
    _, tg, zc = grid(T, D, ctype)
    t = tg if t is None else np.asarray(t).astype(_REAL[ctype])
    bs, nc = np.asarray(bs).astype(ctype), np.asarray(nc).astype(ctype)
    q = np.zeros(D, ctype)
    with np.errstate(all="ignore"):
        q[zc:] = _recursion(bs, nc[:, None] * np.exp(ctype(2j) * bs[:, None] * t[None, zc:]), ctype)
        if zc > 0:
            q[:zc] = np.conj(_recursion(bs, (1 / nc)[:, None] * np.exp(ctype(-2j) * bs[:, None] * t[None, :zc]), ctype))
    return q


# ---- Darboux steps, :864-889 -----------------------------------------------------------------------------------------
def cdt_steps(bs, nc, seed, phi, psi, ctype=np.clongdouble):
    """phi, psi [K, 2, D]: eigenfunctions of the seed at lambda_k -> the seed with K bound states added."""
    bs, nc = np.asarray(bs).astype(ctype), np.asarray(nc).astype(ctype)
    K, D = bs.size, np.asarray(seed).size
    qn = np.asarray(seed).astype(ctype)
    S1, S2 = np.zeros((K, D), ctype), np.zeros((K, D), ctype)
    for i in range(K):
        p1, p2, s1, s2 = phi[i, 0].copy(), phi[i, 1].copy(), psi[i, 0].copy(), psi[i, 1].copy()
        for j in range(i):
            a, ac, b = bs[i] - S1[j], bs[i] - np.conj(S1[j]), S2[j]
            p1, p2 = a * p1 - b * p2, np.conj(b) * p1 + ac * p2
            s1, s2 = a * s1 - b * s2, np.conj(b) * s1 + ac * s2
        beta = (p1 - nc[i] * s1) / (p2 - nc[i] * s2)
        ab = beta.real * beta.real + beta.imag * beta.imag
        S1[i] = (ab * bs[i] + np.conj(bs[i])) / (1 + ab)
        S2[i] = (ctype(2j) * bs[i].imag * beta) / (1 + ab)
        qn = qn - ctype(2j) * S2[i]
    return qn


def cdt_exact_zero_seed_ref(bs, nc, T, D, ctype=np.clongdouble):
    """The pure multi-soliton by Darboux steps on q = 0 with phi = (e^{-i lambda t}, 0), psi = (0, e^{i lambda t})."""
    _, t, _ = grid(T, D, ctype)
    bs = np.asarray(bs).astype(ctype)
    K = bs.size
    phi, psi = np.zeros((K, 2, D), ctype), np.zeros((K, 2, D), ctype)
    with np.errstate(all="ignore"):
        phi[:, 0] = np.exp(ctype(-1j) * bs[:, None] * t[None, :])
        psi[:, 1] = np.exp(ctype(1j) * bs[:, None] * t[None, :])
        return cdt_steps(bs, nc, np.zeros(D, ctype), phi, psi, ctype)


# ---- eigenfunctions of the seed, :908-1007 ---------------------------------------------------------------------------
def step_coefficients(bs, q, h, ctype=np.clongdouble, skip_ks_zero=False):
    """ch, sh [K, D] of the half step h at every sample: U = [[ch - i l sh, q sh], [-q* sh, ch + i l sh]],
    ks = -|q|^2 - l^2, ch = cosh(k h), sh = sinh(k h)/k; at ks == 0 the limit ch = 1, sh = h -- or, with skip_ks_zero,
    the reference's identity step (ch = 1, sh = 0)."""
    rt = _REAL[ctype]
    bs, q = np.asarray(bs).astype(ctype), np.asarray(q).astype(ctype)
    l = bs[:, None]
    ks = -(q.real * q.real + q.imag * q.imag)[None, :] - l * l
    zero = ks == 0
    k = np.sqrt(np.where(zero, ctype(1), ks))
    ch = np.where(zero, ctype(1), np.cosh(k * rt(h)))
    sh = np.where(zero, ctype(0 if skip_ks_zero else h), np.sinh(k * rt(h)) / k)
    return ch, sh


def eigenfunctions_ref(bs, q, T, ctype=np.clongdouble, skip_ks_zero=False):
    """phi, psi [K, 2, D] from phi(T0) = (e^{-i l T0}, 0) and psi(T1) = (0, e^{i l T1}): per interval two half steps of
    eps_t / 2, with sample n-1 then sample n forwards, and their exact inverses (det U = 1: the step with -h) in the
    opposite order backwards.  bs: sorted bound states."""
    rt = _REAL[ctype]
    q = np.asarray(q).astype(ctype)
    D = q.size
    bs = np.asarray(bs).astype(ctype)
    K = bs.size
    eps_t = (float(T[1]) - float(T[0])) / (D - 1)
    ch, sh = step_coefficients(bs, q, eps_t / 2, ctype, skip_ks_zero)
    il = ctype(1j) * bs[:, None] * sh
    a, d = ch - il, ch + il                  # U = [[a, b], [c, d]], U^-1 = [[d, -b], [-c, a]]
    b, c = q[None, :] * sh, -np.conj(q)[None, :] * sh
    phi, psi = np.zeros((K, 2, D), ctype), np.zeros((K, 2, D), ctype)
    p1, p2 = np.exp(ctype(-1j) * bs * rt(T[0])), np.zeros(K, ctype)
    phi[:, 0, 0], phi[:, 1, 0] = p1, p2
    for n in range(1, D):
        for m in (n - 1, n):
            p1, p2 = a[:, m] * p1 + b[:, m] * p2, c[:, m] * p1 + d[:, m] * p2
        phi[:, 0, n], phi[:, 1, n] = p1, p2
    s1, s2 = np.zeros(K, ctype), np.exp(ctype(1j) * bs * rt(T[1]))
    psi[:, 0, D - 1], psi[:, 1, D - 1] = s1, s2
    for n in range(D - 1, 0, -1):
        for m in (n, n - 1):
            s1, s2 = d[:, m] * s1 - b[:, m] * s2, -c[:, m] * s1 + a[:, m] * s2
        psi[:, 0, n - 1], psi[:, 1, n - 1] = s1, s2
    return phi, psi


def cdt_ref(bs, nc, seed, T, ctype=np.clongdouble, skip_ks_zero=False):
    """bs, nc: prepared().  Darboux steps on the seed from its half-step eigenfunctions."""
    with np.errstate(over="ignore", invalid="ignore"):
        phi, psi = eigenfunctions_ref(bs, seed, T, ctype, skip_ks_zero)
        return cdt_steps(bs, nc, seed, phi, psi, ctype)


# ---- a second association of the eigenfunctions: the kernels' chunks -------------------------------------------------
def _mm(A, B):
    """[K, 2, 2] x [K, 2, 2], element type kept (np.matmul has no BLAS path to fall into for long double)."""
    return np.stack([np.stack([A[:, 0, 0] * B[:, 0, 0] + A[:, 0, 1] * B[:, 1, 0], A[:, 0, 0] * B[:, 0, 1] + A[:, 0, 1] * B[:, 1, 1]], 1),
                     np.stack([A[:, 1, 0] * B[:, 0, 0] + A[:, 1, 1] * B[:, 1, 0], A[:, 1, 0] * B[:, 0, 1] + A[:, 1, 1] * B[:, 1, 1]], 1)], 1)


def _mv(A, v):
    return np.stack([A[:, 0, 0] * v[:, 0] + A[:, 0, 1] * v[:, 1], A[:, 1, 0] * v[:, 0] + A[:, 1, 1] * v[:, 1]], 1)


def eigenfunctions_chunked(bs, q, T, ctype=np.complex128, chunk=16, lanes=256):
    """The same eigenfunctions in the association of the kernels (nft_bs_eigenfunctions): the half-step signal
    q'[i] = q[(i + 1) // 2] of 2 (D - 1) samples in chunks of `chunk`; a map per chunk; every lane of body_bs_combine
    composes its run of ceil(nchunk / lanes) chunk maps, one lane carries the vector over the runs, the runs are walked
    again to the chunk boundaries, and the chunks are stepped from their boundary vectors.  The backward steps are the
    step with -h (exp(-A h)), last sample first."""
    rt = _REAL[ctype]
    q = np.asarray(q).astype(ctype)
    D = q.size
    bs = np.asarray(bs).astype(ctype)
    K = bs.size
    eps_t = (float(T[1]) - float(T[0])) / (D - 1)
    D2 = 2 * (D - 1)
    idx = (np.arange(D2) + 1) // 2
    ch, sh = step_coefficients(bs, q, eps_t / 2, ctype)
    il = ctype(1j) * bs[:, None] * sh
    Uf = np.zeros((D2, K, 2, 2), ctype)      # forward step of half-step sample i
    Uf[:, :, 0, 0], Uf[:, :, 1, 1] = (ch - il).T[idx], (ch + il).T[idx]
    Uf[:, :, 0, 1], Uf[:, :, 1, 0] = (q[None, :] * sh).T[idx], (-np.conj(q)[None, :] * sh).T[idx]
    Ub = np.zeros((D2, K, 2, 2), ctype)      # the step with -h: ch even, sh odd in h
    Ub[:, :, 0, 0], Ub[:, :, 1, 1] = Uf[:, :, 1, 1], Uf[:, :, 0, 0]
    Ub[:, :, 0, 1], Ub[:, :, 1, 0] = -Uf[:, :, 0, 1], -Uf[:, :, 1, 0]
    nchunk = (D2 + chunk - 1) // chunk
    G = (nchunk + lanes - 1) // lanes
    eye = np.zeros((K, 2, 2), ctype)
    eye[:, 0, 0] = eye[:, 1, 1] = 1
    bounds = [(c * chunk, min(D2, (c + 1) * chunk)) for c in range(nchunk)]
    runs = [(min(nchunk, g * G), min(nchunk, (g + 1) * G)) for g in range(lanes)]
    phi, psi = np.zeros((K, 2, D), ctype), np.zeros((K, 2, D), ctype)

    # forward
    cm = []
    for n0, n1 in bounds:
        M = eye
        for n in range(n0, n1):
            M = _mm(Uf[n], M)
        cm.append(M)
    gm = []
    for k0, k1 in runs:
        M = eye
        for k in range(k0, k1):
            M = _mm(cm[k], M)
        gm.append(M)
    v = np.stack([np.exp(ctype(-1j) * bs * rt(T[0])), np.zeros(K, ctype)], 1)
    bnd = [None] * nchunk
    for g, (k0, k1) in enumerate(runs):
        p = v
        for k in range(k0, k1):
            bnd[k] = p
            p = _mv(cm[k], p)
        v = _mv(gm[g], v)
    for c, (n0, n1) in enumerate(bounds):
        p = bnd[c]
        if c == 0:
            phi[:, :, 0] = p
        for n in range(n0, n1):
            p = _mv(Uf[n], p)
            if (n + 1) % 2 == 0:
                phi[:, :, (n + 1) // 2] = p

    # backward
    cm = []
    for n0, n1 in bounds:
        M = eye
        for n in range(n1 - 1, n0 - 1, -1):
            M = _mm(Ub[n], M)
        cm.append(M)
    gm = []
    for k0, k1 in runs:
        M = eye
        for k in range(k1 - 1, k0 - 1, -1):
            M = _mm(cm[k], M)
        gm.append(M)
    s = np.stack([np.zeros(K, ctype), np.exp(ctype(1j) * bs * rt(T[1]))], 1)
    bndp = [None] * (nchunk + 1)
    for g in range(lanes - 1, -1, -1):
        k0, k1 = runs[g]
        p = s
        for k in range(k1 - 1, k0 - 1, -1):
            bndp[k + 1] = p
            p = _mv(cm[k], p)
        s = _mv(gm[g], s)
    for c, (n0, n1) in enumerate(bounds):
        p = bndp[c + 1]
        if n1 == D2:
            psi[:, :, D - 1] = p
        for n in range(n1 - 1, n0 - 1, -1):
            p = _mv(Ub[n], p)
            if n % 2 == 0:
                psi[:, :, n // 2] = p
    return phi, psi
