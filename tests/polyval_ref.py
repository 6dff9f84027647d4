"""References for the polynomial evaluation seams (fnft__poly_eval, fnft__poly_evalderiv, fnft_amd_poly_eval_device) and
for the NSE spectrum at arbitrary lambda (fnft_amd_nsev_eval_device).  Helper module, not a test.

(a) eval_ld: p(z) and p'(z) by Horner's scheme in np.clongdouble -- in z where |z| <= 1, on the reversed polynomial in
    x = 1/z where |z| > 1 (p(z) = z^n q(x), p'(z) = z^(n-1) (n q(x) - x q'(x))) -- together with the scales
        S(z) = sum_k |c_k| |z|^k   and   S1(z) = sum_k k |c_k| |z|^(k-1)
    that the errors are measured against.  The value half of the recurrence is tests/roots_ref.py's _horner.
    Accuracy: Horner's scheme in long double errs by at most 2 n 2^-64 S; 1/z rounded to 2^-64 moves q by
    2^-64 |x q'(x)| <= n 2^-64 S.  The power z^n of the outside points would lose n 2^-64 / 2 by repeated squaring in
    long double, 16 u at n = 2^16; it is formed by mpmath in 160 bits and rounded once.
(b) eval_dbl: the reference's own operation order (src/private/fnft__poly_eval.c:25-91: tmp = p[j] + tmp*z, or
    tmp = p[deg-j] + tmp/z and the power z^deg) in complex128.

error(got, ref, scale) is the figure of the tests: |got - ref| / scale at every point, in double after the long-double
subtraction.  bound(e_dbl, floor) = max(MARGIN e_dbl, floor): MARGIN = 4 is tests/slow_cases.py's (another summation
order, 1-2 ulp device functions), FLOOR_POLY = 4 u (the final rounding of a value is at most u S, of the join's sums a
few more) and FLOOR_NSE = 8 u (exp and sincos on top).  check_poly applies the bound to all points together, as the
figure is defined, and to the points of each regime against that regime's own e_dbl.

nse_ld / nse_dbl: a = H11(z) 2^W exp(i lambda pf_a), b = H21(z) 2^W exp(i lambda pf_b) and their lambda-derivatives
(dz/dlambda = i k z, k = 2 eps_t / deg1) from a plan's OWN exported matrix (coefficients and W), so the tree's error is
not in the figure; z = exp(2i lambda eps_t/deg1), pf as NftPlan::run_contspec_impl forms them in double (nse_consts).
Scales: S 2^W |exp(i lambda pf)| for a value, (k |z| S1 + |pf| S) 2^W |exp(i lambda pf)| for a derivative -- the image
of the two polynomial scales under the chain rule.

Long evaluations are spread over threads (numpy releases the GIL inside its loops)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from roots_ref import CLD, LD, U, _horner

MARGIN = 4.0
FLOOR_POLY = 4.0 * U
FLOOR_NSE = 8.0 * U
_THREADS = 16
_PAR_WORK = 1 << 22     # points x coefficients above which an evaluation is spread over threads


def bound(e_dbl, floor):
    return max(MARGIN * e_dbl, floor)


def error(got, ref, scale):
    """|got - ref| / scale per point (float64 array); ref and scale in long double."""
    return (np.abs(np.asarray(got).astype(CLD) - ref) / scale).astype(np.float64)


def _spread(fn, z, work):
    """fn(chunk of z) -> tuple of arrays, concatenated over chunks; threads when the work is large."""
    z = np.asarray(z)
    if work < _PAR_WORK or z.size < 2 * _THREADS:
        return fn(z)
    parts = np.array_split(np.arange(z.size), _THREADS)
    with ThreadPoolExecutor(_THREADS) as ex:
        res = list(ex.map(lambda idx: fn(z[idx]), parts))
    return tuple(np.concatenate([r[k] for r in res]) for k in range(len(res[0])))


def _horner_deriv(c, x, deriv):
    """(p, p', S, S1) of c (highest power first) at the clongdouble vector x; p' and S1 zero without deriv."""
    if not deriv:
        p, s = _horner(c, x)
        return p, np.zeros(x.shape, CLD), s, np.zeros(x.shape, LD)
    ax = np.abs(x)
    p = np.zeros(x.shape, CLD)
    d = np.zeros(x.shape, CLD)
    s = np.zeros(x.shape, LD)
    s1 = np.zeros(x.shape, LD)
    for cj, aj in zip(c.astype(CLD), np.abs(c.astype(CLD))):
        d = d * x + p
        p = p * x + cj
        s1 = s1 * ax + s
        s = s * ax + aj
    return p, d, s, s1


def _pow_exact(z, n):
    """z^n (clongdouble vector, n >= 0) rounded once to long double, through mpmath."""
    import mpmath

    def up(x):      # long double -> mpf, exactly (64 bits in two doubles)
        h = float(x)
        return mpmath.mpf(h) + mpmath.mpf(float(x - LD(h)))

    def down(x):    # mpf -> long double
        h = float(x)
        return LD(h) + LD(float(x - h))

    out = np.zeros(z.shape, CLD)
    with mpmath.workprec(160):
        for i, zi in enumerate(z):
            w = mpmath.mpc(up(zi.real), up(zi.imag)) ** int(n)
            out[i] = CLD(down(w.real)) + 1j * CLD(down(w.imag))
    return out


def _eval_ld_chunk(c, zl, deriv):
    n = c.size - 1
    val = np.zeros(zl.shape, CLD)
    der = np.zeros(zl.shape, CLD)
    sv = np.zeros(zl.shape, LD)
    sd = np.zeros(zl.shape, LD)
    inside = np.abs(zl) <= 1
    if inside.any():
        val[inside], der[inside], sv[inside], sd[inside] = _horner_deriv(c, zl[inside], deriv)
    out = ~inside
    if out.any():
        x = CLD(1) / zl[out]
        q, dq, s, s1 = _horner_deriv(c[::-1], x, deriv)
        zn1 = _pow_exact(zl[out], max(n - 1, 0))
        zn = zn1 * zl[out] if n > 0 else zn1
        val[out] = q * zn
        sv[out] = s * np.abs(zn)
        if deriv:
            der[out] = zn1 * (LD(n) * q - x * dq)
            sd[out] = np.abs(zn1) * (LD(n) * s - np.abs(x) * s1)
    return val, der, sv, sd


def eval_ld(c, z, deriv=True):
    """(p(z), p'(z), S(z), S1(z)) in long double; c: complex128 coefficients, highest power first; z: complex128 or
    clongdouble points."""
    c = np.asarray(c, np.complex128).ravel()
    z = np.asarray(z).ravel().astype(CLD)
    return _spread(lambda zz: _eval_ld_chunk(c, zz, deriv), z, c.size * z.size)


def _eval_dbl_chunk(c, z, deriv):
    deg = c.size - 1
    val = np.zeros(z.shape, np.complex128)
    der = np.zeros(z.shape, np.complex128)
    inside = np.abs(z) <= 1.0
    with np.errstate(all="ignore"):
        for sel, inv in ((inside, False), (~inside, True)):
            if not sel.any():
                continue
            zz = z[sel]
            tmp = np.full(zz.shape, c[deg] if inv else c[0])
            tmp2 = np.zeros(zz.shape, np.complex128)
            for j in range(1, deg + 1):
                if deriv:
                    tmp2 = tmp + (tmp2 / zz if inv else tmp2 * zz)
                tmp = (c[deg - j] + tmp / zz) if inv else (c[j] + tmp * zz)
            if inv:
                der[sel] = zz ** (deg - 1) * (deg * tmp - tmp2 / zz) if deriv else 0.0   # :86
                val[sel] = tmp * zz ** deg                                               # :48, :87
            else:
                val[sel], der[sel] = tmp, tmp2
    return val, der


def eval_dbl(c, z, deriv=True):
    """(p(z), p'(z)) in the reference's operation order, complex128."""
    c = np.asarray(c, np.complex128).ravel()
    z = np.asarray(z, np.complex128).ravel()
    return _spread(lambda zz: _eval_dbl_chunk(c, zz, deriv), z, c.size * z.size)


def poly_errors(c, z, val, der=None):
    """The figures of one polynomial at the points z: e, e_dbl for the values and, der given, ed, ed_dbl for the
    derivatives -- each the maximum over ALL points of |x - long double| / scale, for the product's values (val, der)
    and for eval_dbl's -- and the same per regime of src/private/fnft__poly_eval.c, keys with the suffix _in (|z| <= 1)
    and _out (|z| > 1), where the regime has a point.  The regimes are kept apart because e_dbl of a mixed point set is
    set by the power z^deg of its outside points (cpow: hundreds of u at deg = 500) and would excuse that much on the
    inside points too."""
    deriv = der is not None
    z = np.asarray(z, np.complex128).ravel()
    lv, ldv, sv, sd = eval_ld(c, z, deriv)
    dv, dd = eval_dbl(c, z, deriv)
    ev, ev_dbl = error(val, lv, sv), error(dv, lv, sv)
    inside = np.abs(z) <= 1.0
    out = {}
    groups = (("", np.ones(z.shape, bool)), ("_in", inside), ("_out", ~inside))
    for suf, sel in groups:
        if sel.any():
            out["e" + suf], out["e_dbl" + suf] = float(np.max(ev[sel])), float(np.max(ev_dbl[sel]))
    if deriv:
        ok = sd > 0      # degree 0: the derivative and its scale are zero, and the product must return exactly that
        assert np.all(np.asarray(der)[~ok] == 0)
        sds = np.where(ok, sd, LD(1))
        ed, ed_dbl = error(der, ldv, sds), error(dd, ldv, sds)
        for suf, sel in groups:
            if (sel & ok).any():
                out["ed" + suf], out["ed_dbl" + suf] = float(np.max(ed[sel & ok])), float(np.max(ed_dbl[sel & ok]))
            elif sel.any():
                out["ed" + suf] = out["ed_dbl" + suf] = 0.0
    return out


def check_poly(f, floor=FLOOR_POLY):
    """Asserts e <= max(MARGIN e_dbl, floor) for every figure of poly_errors (merged over polynomials by the caller):
    over all points, and within each regime against that regime's own e_dbl."""
    for k, v in f.items():
        if "_dbl" not in k:
            base, _, suf = k.partition("_")
            ref = f[base + "_dbl" + ("_" + suf if suf else "")]
            assert v <= bound(ref, floor), (k, v / U, ref / U, {a: b / U for a, b in f.items()})


# ---- NSE layer ---------------------------------------------------------------------------------------------------
def nse_consts(T, D, deg0, ups, shifted):
    """(eps_t, deg1, pf_a, pf_b, T1 of the kept steps) as NftPlan::run_contspec_impl forms them in double (nft_plan.h; fnft_nsev.c:766-774,
    fnft__nse_discretization.c:240-379, boundary coefficient 0.5).  D: samples per signal as given (upsampling 1 per kept
    step is the caller's, the tree's D is ups * D); T: their interval."""
    deg1 = float(deg0 * ups)
    Dg = D
    T0, T1 = float(T[0]), float(T[1])
    if ups != 1:
        T1 = T0 + float(Dg - 1) * ((T1 - T0) / float(D - 1))
    eps_t = (T1 - T0) / float(Dg - 1)
    sh = eps_t / deg1 if shifted else 0.0
    pf_a = -eps_t * float(Dg) + (T1 + eps_t * 0.5) - (T0 - eps_t * 0.5)
    pf_b = -eps_t * float(Dg) - (T1 + eps_t * 0.5) - (T0 - eps_t * 0.5) + sh
    return eps_t, deg1, pf_a, pf_b, T1


def nse_ld(tm, W, lam, consts, deriv):
    """Long double a, b (and da, db) of the matrix tm [4, deg+1] * 2^W at lam, with their scales:
    dict(a, b, da, db, sa, sb, sda, sdb)."""
    eps_t, deg1, pf_a, pf_b = consts[:4]
    lam = np.asarray(lam, np.complex128).ravel()
    ll = lam.astype(CLD)
    k = 2 * LD(eps_t) / LD(deg1)
    zl = np.exp(1j * ll * k)
    s2 = np.ldexp(LD(1), int(W))
    out = {}
    for name, row, pf in (("a", 0, pf_a), ("b", 2, pf_b)):
        v, d, sv, sd = eval_ld(tm[row], zl, True)
        E = np.exp(1j * ll * LD(pf)) * s2
        out[name] = v * E
        out["s" + name] = sv * np.abs(E)
        if deriv:
            out["d" + name] = (1j * k * zl * d + 1j * LD(pf) * v) * E
            out["sd" + name] = (k * np.abs(zl) * sd + abs(LD(pf)) * sv) * np.abs(E)
    return out


def nse_dbl(tm, W, lam, consts, deriv):
    """The same formulas in double: z = exp(2i lambda eps_t/deg1) as fnft__akns_discretization.c:217 forms it, the
    polynomial by eval_dbl, exp(i lambda pf) and 2^W."""
    eps_t, deg1, pf_a, pf_b = consts[:4]
    lam = np.asarray(lam, np.complex128).ravel()
    z = np.exp(2j * lam * eps_t / deg1)
    out = {}
    for name, row, pf in (("a", 0, pf_a), ("b", 2, pf_b)):
        v, d = eval_dbl(tm[row], z, deriv)
        E = np.exp(1j * lam * pf)
        out[name] = np.ldexp(1.0, int(W)) * (v * E)
        if deriv:
            out["d" + name] = np.ldexp(1.0, int(W)) * ((d * (2j * eps_t / deg1 * z) + 1j * pf * v) * E)
    return out


def nse_errors(tm, W, lam, consts, got, deriv):
    """got: one signal's output of the eval call, [a | b] or [a | b | da | db] of n points.  Returns
    dict(e, e_dbl, ref): the maxima over all points and parts of |x - long double| / scale, and the long-double values."""
    n = np.asarray(lam).size
    ref = nse_ld(tm, W, lam, consts, deriv)
    dbl = nse_dbl(tm, W, lam, consts, deriv)
    names = ["a", "b"] + (["da", "db"] if deriv else [])
    e = e_dbl = 0.0
    for k, name in enumerate(names):
        e = max(e, float(np.max(error(got[k * n:(k + 1) * n], ref[name], ref["s" + name]))))
        e_dbl = max(e_dbl, float(np.max(error(dbl[name], ref[name], ref["s" + name]))))
    return dict(e=e, e_dbl=e_dbl, ref=ref)


def grid_shift(tm_row, A, V, xi, consts):
    """The chirp transform evaluates at z_m = V^m / A for the DOUBLES A = exp(i phi_A), V = exp(i phi_V) the host forms
    (fnft_nsev.c:822-827; tests/chirp_ref.nsev_grid), the evaluation at z = exp(2i xi_m eps_t/deg1): the same points only
    up to the rounding of A and V, m times over for V.  Returns max_m |p'(z_m)| |dz_m| / S(z_m) for the polynomial
    tm_row -- what that difference of the points is worth in the figure of the tests, beyond either side's own error."""
    from chirp_ref import ld_log
    eps_t, deg1 = consts[0], consts[1]
    la, lv = ld_log(A), ld_log(V)
    m = np.arange(len(xi)).astype(LD)
    z_cs = np.exp((m * lv[0] - la[0]) + 1j * (m * lv[1] - la[1]).astype(CLD))
    z_ev = np.exp(1j * np.asarray(xi).astype(CLD) * (2 * LD(eps_t) / LD(deg1)))
    _, d, sv, _ = eval_ld(tm_row, z_ev, True)
    return float(np.max(np.abs(d) * np.abs(z_cs - z_ev) / sv))


def chirp_term(A, V, deg, M, xi, consts):
    """What the plan's chirp transform may differ from the long-double value AT ITS OWN POINTS, in the figure of the
    tests: chirp_ref.err_bound with chirp_cases.BOUND_NSE, u (A log2 L + P Phi), L the transform length (at least 8192).
    Phi is the largest phase a chirp factor that multiplies data is rounded at: their indices stay below deg + M (the
    filter's), not L, so Phi = phi(deg + M) -- for a short polynomial thousands of times below chirp_ref.phi(L) -- plus
    the phase of exp(i xi pf)."""
    import chirp_cases as CC
    import chirp_ref as CR
    L = max(2 * CC.ROW, 1 << int(np.ceil(np.log2(deg + M))))
    phi_pf = float(np.max(np.abs(xi)) * max(abs(consts[2]), abs(consts[3])))
    return CR.err_bound(CC.BOUND_NSE, L, CR.phi(deg + M, A, V) + phi_pf)


def own_grid_check(tm, W, T1, T, XI, M, D, consts, got, cs):
    """Real lambda on a plan's own xi-grid: `got` ([a(M) | b(M)] of the evaluation) against `cs` (the plan's contspec of
    type AB) -- the only check of the phase factors and of the map lambda -> z that does not restate them, since the
    chirp transform forms its own.  Bound per part: the evaluation's max(MARGIN e_dbl, FLOOR_NSE), plus chirp_term, plus
    grid_shift.  T1: the end of the interval the tree's steps span (T[1] for upsampling 1).  Prints the figures."""
    import chirp_ref as CR
    eps_t, deg1 = consts[0], consts[1]
    xi = XI[0] + (XI[1] - XI[0]) / (M - 1) * np.arange(M)
    ref = nse_ld(tm, W, xi, consts, False)
    dbl = nse_dbl(tm, W, xi, consts, False)
    A, V = CR.nsev_grid((T[0], T1), XI, M, D, int(deg1))
    b_chirp = chirp_term(A, V, tm.shape[1] - 1, M, xi, consts)
    for k, name in enumerate(("a", "b")):
        e_dbl = float(np.max(error(dbl[name], ref[name], ref["s" + name])))
        shift = grid_shift(tm[2 * k], A, V, xi, consts)
        d = float(np.max(error(got[k * M:(k + 1) * M], np.asarray(cs[k * M:(k + 1) * M]).astype(CLD), ref["s" + name])))
        print(name, "eval - contspec %.2f u; bounds: eval %.2f u + chirp %.2f u + points %.2f u" % (
            d / U, bound(e_dbl, FLOOR_NSE) / U, b_chirp / U, shift / U))
        assert d <= bound(e_dbl, FLOOR_NSE) + b_chirp + shift, name
