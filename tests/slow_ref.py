"""Extended-precision restatement of fnft_nsev's continuous spectrum under the slow discretizations (BO, CF4_2, CF4_3,
CF5_3, CF6_4, ES4, TES4): a helper, not a test.  It follows the reference line by line --

  preprocessing     src/private/fnft__nse_discretization.c:390-655 (resampling: src/private/fnft__misc.c:326-407)
  weights           src/private/fnft__akns_discretization.c:243-381
  step matrices     src/private/fnft__akns_scatter_matrix.c:112-241 (CF family), :259-304 and :456-528 (ES4, TES4)
  boundary, phases  src/fnft_nsev.c:763-891, src/private/fnft__nse_discretization.c:240-375
  Richardson        src/fnft_nsev.c:316-406

-- in numpy, vectorised over the xi-grid.  dtype=np.clongdouble (the default) is the ground truth of the GPU and
emulator tests; dtype=np.complex128 runs the same code in double, which is the reference's own arithmetic and what the
tests calibrate their tolerance against.  np.fft keeps complex256, so the resampler is the FFT in both."""
import numpy as np

DISCS = ("BO", "CF4_2", "CF4_3", "CF5_3", "CF6_4", "ES4", "TES4")
UPSAMPLING = {"BO": 1, "CF4_2": 2, "CF4_3": 3, "CF5_3": 3, "CF6_4": 4, "ES4": 3, "TES4": 3}
ORDER = {"BO": 2, "CF4_2": 4, "CF4_3": 4, "CF5_3": 5, "CF6_4": 6, "ES4": 4, "TES4": 4}


def _real(dtype):
    return np.longdouble if np.dtype(dtype) == np.dtype(np.clongdouble) else np.float64


def _round(x):
    return int(np.floor(float(x) + 0.5))     # C round() for positive arguments


def _legendre(n, x):
    if n == 0:
        return x * 0 + 1
    if n == 1:
        return x
    p1, p2 = x, x * 0 + 1
    for i in range(2, n + 1):
        p = (2.0 * i - 1) * x * p1 / i - (i - 1.0) * p2 / i
        p2, p1 = p1, p
    return p


def weights(disc, dtype=np.clongdouble):
    """(w[rows][cols] resampling weights, l_weights[rows], shift in steps of the two resampled copies or None)."""
    R = _real(dtype)
    Z = np.dtype(dtype).type
    if disc == "BO":
        return np.ones((1, 1), dtype), np.ones(1, dtype), None
    if disc in ("ES4", "TES4"):
        return None, None, None
    if disc == "CF4_2":
        s = np.sqrt(R(3)) / R(6)
        w = np.array([[R(0.25) + s, R(0.25) - s], [R(0.25) - s, R(0.25) + s]], dtype)
        shift = s
    elif disc == "CF4_3":
        f = [[R(11) / R(40), R(20) / R(87), R(7) / R(50)], [R(9) / R(20), R(0), -R(7) / R(25)],
             [R(11) / R(40), -R(20) / R(87), R(7) / R(50)]]
        wm = [R(5) / R(18), R(4) / R(9), R(5) / R(18)]
        xm = [R(2) * np.sqrt(R(3) / R(20)), R(0), -R(2) * np.sqrt(R(3) / R(20))]
        w = np.zeros((3, 3), dtype)
        for m in range(3):
            for i in range(3):
                a = Z(0)
                for n in range(3):
                    a = a + (2 * n + 1) * _legendre(n, xm[m]) * f[i][n]
                w[i, m] = a * wm[m]
        shift = np.sqrt(R(3) / R(20))
    elif disc == "CF5_3":
        s15 = np.sqrt(R(15))
        w0 = Z((R(145) + R(37) * s15) / R(900)) + Z(1j) * ((R(5) + R(3) * s15) / R(300))
        w1 = Z(-R(1) / R(45)) + Z(1j) * (R(1) / R(15))
        w2 = Z((R(145) - R(37) * s15) / R(900)) + Z(1j) * ((R(5) - R(3) * s15) / R(300))
        w3 = Z(-R(2) / R(45)) + Z(1j) * (-s15 / R(50))
        w4 = Z(R(22) / R(45))
        w = np.array([[w0, w1, w2], [w3, w4, np.conj(w3)], [np.conj(w2), np.conj(w1), np.conj(w0)]], dtype)
        shift = s15 / R(10)
    elif disc == "CF6_4":
        c = [0.245985577298764 + 0.038734389227165j, -0.046806149832549 + 0.012442141491185j,
             0.010894359342569 - 0.004575808769067j, 0.062868370946917 - 0.048761268117765j,
             0.269028372054771 - 0.012442141491185j, -0.041970529810473 + 0.014602687659668j]
        flat = c + c[::-1]
        w = np.array(flat, dtype).reshape(4, 3)
        shift = np.sqrt(R(15)) / R(10)
    else:
        raise ValueError(disc)
    lw = np.zeros(w.shape[0], dtype)
    for i in range(w.shape[0]):
        acc = Z(0)
        for j in range(w.shape[1]):
            acc = acc + w[i, j]
        lw[i] = acc
    if disc == "CF4_2":
        lw[1] = lw[0]          # fnft__akns_scatter_matrix.c:128-129
    return w, lw, shift


def resample(q, eps_t, delta, dtype=np.clongdouble):
    """fnft__misc_resample: the periodic continuation of q shifted by delta."""
    R = _real(dtype)
    D = q.size
    X = np.fft.fft(q.astype(dtype))
    assert X.dtype == np.dtype(dtype)
    i = np.arange(D)
    scl = R(D) * R(eps_t)
    freq = np.where(i < D // 2, i.astype(R), i.astype(R) - R(D)) / scl
    X = X * np.exp((1j * (2 * np.arccos(R(-1)) * R(delta) * freq)).astype(dtype))
    out = np.fft.ifft(X)
    assert out.dtype == np.dtype(dtype)
    return out


def preprocess(q, eps_t, kappa, disc, Dsub, dtype=np.clongdouble):
    """fnft__nse_discretization_preprocess_signal: (q_pre, r_pre, Dsub, nskip)."""
    R = _real(dtype)
    q = np.asarray(q).astype(dtype)
    D = q.size
    eps_t = R(eps_t)
    Dsub = min(max(int(Dsub), 2), D)
    nskip = _round(D / Dsub)
    Dsub = _round(D / nskip)
    ups = UPSAMPLING[disc]
    idx = np.arange(Dsub) * nskip
    w, _, shift = weights(disc, dtype)
    qp = np.zeros(Dsub * ups, dtype)
    rp = np.zeros(Dsub * ups, dtype)
    rof = lambda x: -kappa * np.conj(x)
    if disc == "BO":
        qp[:] = q[idx]
        rp[:] = rof(qp)
    elif disc in ("CF4_2", "CF4_3", "CF5_3", "CF6_4"):
        assert D > 2
        q1 = resample(q, eps_t, -eps_t * shift * nskip, dtype)
        q3 = resample(q, eps_t, eps_t * shift * nskip, dtype)
        src = [q1, q3] if disc == "CF4_2" else [q1, q, q3]
        for p in range(ups):
            acc_q = w[p, 0] * src[0][idx]
            acc_r = w[p, 0] * rof(src[0][idx])
            for j in range(1, len(src)):
                acc_q = acc_q + w[p, j] * src[j][idx]
                acc_r = acc_r + w[p, j] * rof(src[j][idx])
            qp[p::ups] = acc_q
            # CF4_2, CF4_3: r = -kappa conj(q_pre), which is the same number for real weights
            rp[p::ups] = acc_r if disc in ("CF5_3", "CF6_4") else rof(acc_q)
    else:
        h = eps_t * nskip
        q0 = q[idx]
        z = np.zeros(1, dtype)
        qn = np.concatenate([q0[1:], z])
        qm = np.concatenate([z, q0[:-1]])
        qp[0::3] = q0
        qp[1::3] = (qn - qm) / (2 * h)
        qp[2::3] = (qn - 2 * q0 + qm) / (h * h)
        rp[:] = rof(qp)
    return qp, rp, Dsub, nskip


def _pauli(a1, a2, a3):
    """(c, s) of exp(a1 s1 + a2 s2 + a3 s3) = c + s (a . sigma), fnft__akns_scatter_matrix.c:469-478."""
    w = np.sqrt(-(a1 * a1) - (a2 * a2) - (a3 * a3))
    nz = w != 0
    s = np.where(nz, np.sin(w) / np.where(nz, w, 1), 1)
    return np.cos(w), s


def scatter(qp, rp, eps_t, xi, disc, dtype=np.clongdouble):
    """First column (S11, S21) of akns_scatter_matrix's product at every xi."""
    R = _real(dtype)
    Z = np.dtype(dtype).type
    e = R(eps_t)
    xi = np.asarray(xi).astype(dtype)
    t0 = np.ones(xi.size, dtype)
    t1 = np.zeros(xi.size, dtype)
    I = Z(1j)

    def push(u00, u01, u10, u11):
        nonlocal t0, t1
        t0, t1 = u00 * t0 + u01 * t1, u10 * t0 + u11 * t1

    if disc in ("BO", "CF4_2", "CF4_3", "CF5_3", "CF6_4"):
        _, lw, _ = weights(disc, dtype)
        N = UPSAMPLING[disc]
        for n in range(qp.size):
            l = xi * lw[n % N]
            ks = qp[n] * rp[n] - l * l
            k = np.sqrt(ks)
            ch = np.cosh(k * e)
            nz = ks != 0
            sh = np.where(nz, np.sinh(k * e) / np.where(nz, k, 1), e)
            u1 = l * sh * I
            push(ch - u1, qp[n] * sh, rp[n] * sh, ch + u1)
        return t0, t1
    e3, e2 = e * e * e, e * e
    for n in range(0, qp.size, 3):
        q0, q1, q2 = qp[n], qp[n + 1], qp[n + 2]
        r0, r1, r2 = rp[n], rp[n + 1], rp[n + 2]
        if disc == "ES4":
            tm0 = e3 * (q2 + r2) / 48 + (e * (q0 + r0)) * R(0.5)
            tm1 = (e * (q0 - r0) * I) * R(0.5) + (e3 * (q2 - r2) * I) / 48
            tm2 = -e3 * (q0 * r1 - q1 * r0) / 12
            a1 = tm0 + e3 * (xi * I * (q1 - r1)) / 12
            a2 = tm1 - e3 * xi * (q1 + r1) / 12
            a3 = -e * I * xi + tm2
            c, s = _pauli(a1, a2, a3)
            push(c + s * a3, s * (a1 - I * a2), s * (a1 + I * a2), c - s * a3)
        else:
            zero = np.zeros(xi.size, dtype)
            steps = [((e3 * (q2 + r2)) / 96 - (e2 * (q1 + r1)) / 24 + zero,
                      (e3 * (q2 - r2) * I) / 96 + (e2 * (r1 - q1) * I) / 24 + zero, zero),
                     ((e * (q0 + r0)) * R(0.5) + zero, (e * (q0 * I - r0 * I)) * R(0.5) + zero, -e * xi * I),
                     ((e3 * (q2 + r2)) / 96 + (e2 * (q1 + r1)) / 24 + zero,
                      (e3 * (q2 - r2) * I) / 96 + (e2 * (q1 - r1) * I) / 24 + zero, zero)]
            for a1, a2, a3 in steps:
                c, s = _pauli(a1, a2, a3)
                push(c + s * a3, s * (a1 - I * a2), s * (a1 + I * a2), c - s * a3)
    return t0, t1


def contspec(qp, rp, Dg, T, xi, disc, dtype=np.clongdouble):
    """nsev_compute_contspec for a slow scheme: (rho, a, b); Dg kept grid points on [T[0], T[1]]."""
    R = _real(dtype)
    T0, T1 = R(T[0]), R(T[1])
    eps_t = (T1 - T0) / (Dg - 1)
    h11, h21 = scatter(qp, rp, eps_t, xi, disc, dtype)
    xi = np.asarray(xi).astype(dtype)
    bc = R(0.5)
    pf_rho = -2 * (T1 + eps_t * bc)
    pf_a = (T1 + eps_t * bc) - (T0 - eps_t * bc)
    pf_b = -(T1 + eps_t * bc) - (T0 - eps_t * bc)
    I = np.dtype(dtype).type(1j)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = h21 * np.exp(I * xi * pf_rho) / h11
    return rho, h11 * np.exp(I * xi * pf_a), h21 * np.exp(I * xi * pf_b)


def nsev_slow(q, T, M, XI, kappa, disc, richardson=0, dtype=np.clongdouble):
    """fnft_nsev's contspec with opts->discretization = disc: dict of 'rho', 'a', 'b' (arrays of M values of dtype)."""
    R = _real(dtype)
    q = np.asarray(q, np.complex128)
    D = q.size
    T0, T1 = R(T[0]), R(T[1])
    eps_t = (T1 - T0) / (D - 1)
    xi = R(XI[0]) + ((R(XI[1]) - R(XI[0])) / (M - 1)) * np.arange(M).astype(R)
    qp, rp, Dsub, nskip = preprocess(q, eps_t, kappa, disc, D, dtype)
    assert Dsub == D and nskip == 1
    X = list(contspec(qp, rp, D, (T0, T1), xi, disc, dtype))
    if richardson:
        qs, rs, Dsub, nskip = preprocess(q, eps_t, kappa, disc, D // 2, dtype)
        Tsub = (T0, T0 + ((Dsub - 1) * nskip) * eps_t)
        eps_sub = (Tsub[1] - Tsub[0]) / (Dsub - 1)
        Y = contspec(qs, rs, Dsub, Tsub, xi, disc, dtype)
        num = (eps_sub / eps_t) ** ORDER[disc]
        den = num - 1
        sel = np.abs(xi) < R(0.9) * np.arccos(R(-1)) / (2 * eps_sub)
        for k in range(3):
            X[k] = np.where(sel, (num * X[k] - Y[k]) / den, X[k])
    return {"rho": X[0], "a": X[1], "b": X[2]}


def rel_max(x, ref):
    """max_m |x - ref| / max_m |ref| in long double."""
    x = np.asarray(x).astype(np.clongdouble)
    ref = np.asarray(ref).astype(np.clongdouble)
    return float(np.abs(x - ref).max() / np.abs(ref).max())
