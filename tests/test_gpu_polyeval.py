"""Polynomials at arbitrary points on the GPU: the host seams fnft__poly_eval / fnft__poly_evalderiv, their batched
device twin fnft_amd_poly_eval_device, and fnft_amd_nsev_eval_device -- a(lambda), b(lambda) and their derivatives of a
plan's transfer matrix (tests/test_polyeval_emu.py is the same in the CPU lane emulator).

Accuracy as in the emulator file: e = |got - long double| / scale (tests/polyval_ref.py), every test asserts the maximum
over ALL of its points, e <= max(MARGIN e_dbl, FLOOR), e_dbl the same figure of the reference's formula run in double,
and the NSE layer applies the formulas to the matrix the plan itself exports (Plan.transfer_matrix)."""
import json
import os

import numpy as np
import pytest

import discspec_batch_cases as DC
import polyeval_cases as PC
import polyval_ref as PR
import signals as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNFT_EC_INVALID_ARGUMENT, FNFT_EC_NOT_YET_IMPLEMENTED = 2, 6
DBL_EPSILON = 2.0 ** -52


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    c.silence_errors()
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.complex128).reshape(-1)).to("cuda")


# ---- the reference's own vector ---------------------------------------------------------------------------------
def test_reference_vector_through_both_host_seams(capi):
    """test/fnft__poly/fnft__poly_eval_test.c: degree 3, one point inside and one outside the unit circle, relative
    error sum |x - exact| / sum |exact| <= 100 DBL_EPSILON for the values and the derivatives."""
    with open(os.path.join(ROOT, "tests", "golden", "poly_eval_fixtures.json")) as f:
        fx = json.load(f)["poly_eval"]
    deg = fx["deg"]
    p, z = S.l2c(fx["p"]), S.l2c(fx["z"])
    exact = np.array([sum(p[j] * zi ** (deg - j) for j in range(deg + 1)) for zi in z])
    dexact = np.array([sum((deg - (j - 1)) * p[j - 1] * zi ** (deg - j) for j in range(1, deg + 1)) for zi in z])
    bound = fx["bound_dbl_epsilon"] * DBL_EPSILON

    def rel(x, ex):
        return float(np.sum(np.abs(x - ex)) / np.sum(np.abs(ex)))

    rc, v = capi.poly_eval(p, z)
    assert rc == 0, capi.last_error()
    rc, v2, d = capi.poly_evalderiv(p, z)
    assert rc == 0, capi.last_error()
    print("rel err: eval %.3e, evalderiv %.3e / %.3e, bound %.3e" % (rel(v, exact), rel(v2, exact), rel(d, dexact), bound))
    assert rel(v, exact) <= bound and rel(v2, exact) <= bound and rel(d, dexact) <= bound
    assert np.array_equal(v, v2)


# ---- polynomial layer --------------------------------------------------------------------------------------------
def poly_run(capi, torch, deg, nz, batch=1, npoly=1, shared=True, pad=0, deriv=True, key=(), rmax=1.5):
    ps, bs = deg + 1 + pad, npoly * (deg + 1 + pad) + pad
    zs = 0 if shared else nz + pad
    p = PC.coefficients(batch * bs, deg, nz, batch, npoly, *key)
    z = PC.points((1 if shared else batch) * (nz + pad), deg, *key, rmax=rmax)
    dp, dz = dev(torch, p), dev(torch, z)
    dv = torch.full((batch * npoly * nz,), float("nan"), dtype=torch.complex128, device="cuda")
    dd = torch.full((batch * npoly * nz,), float("nan"), dtype=torch.complex128, device="cuda") if deriv else None
    rc = capi.poly_eval_device(deg, npoly, batch, dp.data_ptr(), ps, bs, nz, dz.data_ptr(), zs, dv.data_ptr(),
                               dd.data_ptr() if deriv else 0)
    assert rc == 0, capi.last_error()
    assert np.array_equal(dz.cpu().numpy(), z)            # the device twin does not evaluate in place
    val = dv.cpu().numpy().reshape(batch, npoly, nz)
    der = dd.cpu().numpy().reshape(batch, npoly, nz) if deriv else None
    worst = {}
    for b in range(batch):
        zb = z[b * zs:b * zs + nz]
        for j in range(npoly):
            c = p[b * bs + j * ps:b * bs + j * ps + deg + 1]
            f = PR.poly_errors(c, zb, val[b, j], der[b, j] if deriv else None)
            for k, v in f.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("deg %d nz %d batch %d npoly %d:" % (deg, nz, batch, npoly),
          " ".join("%s %.2f u" % (k, v / PR.U) for k, v in sorted(worst.items())))
    PR.check_poly(worst)


@pytest.mark.parametrize("deg", PC.DEGS)
def test_degrees_and_point_counts(capi, torch, deg):
    for nz in PC.NZS:
        poly_run(capi, torch, deg, nz)


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("npoly", (1, 2))
def test_layouts(capi, torch, batch, npoly):
    """Every combination of the emulator's layout test at its shape, and shared / per-signal points with padded strides
    at a shape with a second workgroup and a second tile."""
    for shared in (True, False):
        for pad, deriv in ((0, True), (3, True), (3, False)):
            poly_run(capi, torch, 13, 65, batch=batch, npoly=npoly, shared=shared, pad=pad, deriv=deriv)
        poly_run(capi, torch, PC.TILE + 1, 257, batch=batch, npoly=npoly, shared=shared, pad=3, deriv=shared)


@pytest.mark.parametrize("nz,deriv", [(5, True), (4099, False)])
def test_long_polynomial(capi, torch, nz, deriv):
    """deg = 2^16 + 3: with 5 points the coefficient range is cut into segments (one workgroup of points, so S > 1 by
    polyeval_segments; values and derivatives); with 4099 points 17 workgroups share fewer (values: the long-double
    reference of 4099 x 65540 terms is what this case costs, and the derivative would double it).  |z| <= 1 + 2^-8
    outside the circle, where z^deg still fits a double."""
    poly_run(capi, torch, (1 << 16) + 3, nz, deriv=deriv, rmax=1.0 + 2.0 ** -8)


def test_host_seams_match_the_device_twin(capi, torch):
    """In place on host buffers: the same kernels, so the same bits as the device twin; a longer, segmented call too."""
    for deg, nz in ((9, 65), (5000, 7)):
        p, z = PC.coefficients(deg + 1, "host", deg), PC.points(nz, "host", deg)
        rc, v = capi.poly_eval(p, z)
        rc2, v2, d2 = capi.poly_evalderiv(p, z)
        assert rc == 0 and rc2 == 0, capi.last_error()
        dv = torch.zeros(nz, dtype=torch.complex128, device="cuda")
        dd = torch.zeros(nz, dtype=torch.complex128, device="cuda")
        assert capi.poly_eval_device(deg, 1, 1, dev(torch, p).data_ptr(), deg + 1, deg + 1, nz, dev(torch, z).data_ptr(), 0,
                                     dv.data_ptr(), dd.data_ptr()) == 0
        assert np.array_equal(v2, dv.cpu().numpy()) and np.array_equal(d2, dd.cpu().numpy())
        f = PR.poly_errors(p, z, v)
        PR.check_poly(f)


# ---- NSE layer ---------------------------------------------------------------------------------------------------
T = (-2.0, 2.0)


class EvalPlan:
    """A plan, its signals on the device, and the calls of the tests; every call waits for its result."""

    def __init__(self, capi, torch, disc, D, kappa=1, batch=1, M=0, T=T, q=None):
        self.capi, self.torch, self.disc, self.D, self.kappa, self.B, self.M, self.T = capi, torch, disc, D, kappa, batch, M, T
        self.plan = capi.Plan(D, M, batch=batch, discretization=disc)
        self.q = PC.nse_signal(D, T, batch, disc, kappa) if q is None else np.asarray(q, np.complex128).reshape(batch, D)
        self.dq = dev(torch, self.q)
        self.consts = PR.nse_consts(T, D, PC.DEG0[disc], PC.UPS[disc], disc in ("2SPLIT2_MODAL", "2SPLIT2A"))

    def transform(self, XI=None, finish=True):
        """contspec_device: the AB spectrum [B, 2M] with a grid, the tree alone without."""
        out = None
        if XI is not None:
            out = self.torch.zeros(self.B * 2 * self.M, dtype=self.torch.complex128, device="cuda")
        rc = self.plan.contspec_device(self.dq.data_ptr(), out.data_ptr() if XI is not None else 0, self.T,
                                       XI or (-1.0, 1.0), kappa=self.kappa, contspec_type="AB")
        assert rc == 0, self.capi.last_error()
        if finish:
            assert self.plan.finish() == 0, self.capi.last_error()
        return None if out is None else out.cpu().numpy().reshape(self.B, 2 * self.M)

    def eval(self, lam, deriv, per_signal=False):
        lam = np.ascontiguousarray(lam, np.complex128)
        n = lam.shape[-1]
        dl = dev(self.torch, lam)
        out = self.torch.full((self.B * self.plan.eval_len(n, deriv),), float("nan"), dtype=self.torch.complex128,
                              device="cuda")
        rc = self.plan.eval_device(dl.data_ptr(), n, out.data_ptr(), self.T, derivative=deriv, per_signal=per_signal)
        assert rc == 0, (rc, self.capi.last_error())
        assert self.plan.finish() == 0, self.capi.last_error()
        assert np.array_equal(dl.cpu().numpy(), lam.reshape(-1))
        return out.cpu().numpy().reshape(self.B, -1)

    def check(self, tag, lam, got, deriv):
        lam = np.asarray(lam)
        worst = dict(e=0.0, e_dbl=0.0)
        for b in range(self.B):
            rc, deg, tm, W = self.plan.transfer_matrix(b)
            assert rc == 0
            f = PR.nse_errors(tm, W, lam if lam.ndim == 1 else lam[b], self.consts, got[b], deriv)
            worst = dict(e=max(worst["e"], f["e"]), e_dbl=max(worst["e_dbl"], f["e_dbl"]))
        print(tag, "e %.2f u  e_dbl %.2f u" % (worst["e"] / PR.U, worst["e_dbl"] / PR.U))
        assert worst["e"] <= PR.bound(worst["e_dbl"], PR.FLOOR_NSE), (tag, worst)

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("disc,D,kappa,batch", [("2SPLIT2_MODAL", 8192, 1, 1), ("2SPLIT4B", 256, 1, 1),
                                                ("4SPLIT4B", 64, 1, 1), ("2SPLIT4B", 256, -1, 1),
                                                ("2SPLIT2_MODAL", 512, 1, 3)])
def test_nse_values_and_derivatives(capi, torch, disc, D, kappa, batch):
    """MODAL D = 8192 is a split tree whose root is still pending when eval is called (the chirp transform took it from
    the row kernel); batch = 3 evaluates per-signal points.  Derivative on (complex lambda) and off (real lambda)."""
    M = D if D == 8192 else 0
    P = EvalPlan(capi, torch, disc, D, kappa, batch, M)
    try:
        P.transform(XI=(-2.0, 2.0) if M else None, finish=False)
        per = batch > 1
        lam = np.array([PC.lambdas(301, T, "complex", disc, b) for b in range(batch)]) if per \
            else PC.lambdas(301, T, "complex", disc)
        got = P.eval(lam, True, per_signal=per)
        P.check("%s D %d kappa %d batch %d complex+deriv" % (disc, D, kappa, batch), lam, got, True)
        lam = PC.lambdas(130, T, "real", disc)
        got = P.eval(lam, False)
        P.check("%s D %d kappa %d batch %d real" % (disc, D, kappa, batch), lam, got, False)
    finally:
        P.close()


@pytest.mark.parametrize("disc,D", [("2SPLIT4B", 256), ("4SPLIT4B", 64)])
def test_nse_on_the_plans_own_grid(capi, torch, disc, D):
    """Real lambda on the plan's xi-grid, upsampling 1 and 2: the evaluation against the chirp transform's contspec of
    type AB (polyval_ref.own_grid_check: the evaluation's bound, the chirp transform's at its own points, and what the
    two definitions of the points differ by -- the chirp transform's are powers of the rounded doubles A and V)."""
    M, XI = 300, (-1.5, 2.0)
    P = EvalPlan(capi, torch, disc, D, 1, 1, M)
    try:
        cs = P.transform(XI=XI)
        xi = XI[0] + (XI[1] - XI[0]) / (M - 1) * np.arange(M)
        got = P.eval(xi.astype(np.complex128), False)
        P.check("own grid " + disc, xi, got, False)
        rc, deg, tm, W = P.plan.transfer_matrix(0)
        PR.own_grid_check(tm, W, P.consts[4], T, XI, M, D, P.consts, got[0], cs[0])
    finally:
        P.close()


def test_smaller_n_allocates_nothing_on_a_long_signal(capi, torch):
    """D = 2^20: a segment keeps its 1024 powers up to S = 1024, so S doubles when n drops from 300 (two workgroups of
    points per polynomial) to 256 (one).  The plan's workspace stays what the first call made it, and the values agree
    (other segments, so not bit for bit: to 1e-12 of the largest)."""
    D = 1 << 20
    P = EvalPlan(capi, torch, "2SPLIT2_MODAL", D, 1, 1, 0, q=0.05 * PC.nse_signal(D, T, 1, "long"))
    try:
        P.transform()
        lam = PC.lambdas(300, T, "real", "long")
        e300 = P.eval(lam, True)
        ws = P.plan.workspace_bytes
        e256 = P.eval(lam[:256], True)
        e8 = P.eval(lam[:8], True)
        assert P.plan.workspace_bytes == ws
        for k in range(4):
            a, b, c = e300[0, k * 300:k * 300 + 256], e256[0, k * 256:(k + 1) * 256], e8[0, k * 8:(k + 1) * 8]
            tol = 1e-12 * np.max(np.abs(a))
            assert np.all(np.isfinite(a)) and np.max(np.abs(a - b)) <= tol and np.max(np.abs(a[:8] - c)) <= tol
    finally:
        P.close()


def test_sequence_leaves_the_plan_as_it_was(capi, torch):
    """contspec -> eval -> contspec on one plan gives bitwise the contspec of a fresh plan (D = 8192: the eval resolves a
    pending root in between), eval twice gives identical bits, and a second eval allocates nothing."""
    disc, D, M, XI = "2SPLIT2_MODAL", 8192, 8192, (-2.0, 2.0)
    lam = PC.lambdas(257, T, "complex", "seq")
    fresh = EvalPlan(capi, torch, disc, D, 1, 2, M)
    P = EvalPlan(capi, torch, disc, D, 1, 2, M)
    try:
        want = fresh.transform(XI=XI)
        first = P.transform(XI=XI)
        e1 = P.eval(lam, True)
        ws = P.plan.workspace_bytes
        e2 = P.eval(lam, True)
        e3 = P.eval(lam[:100], False)
        assert P.plan.workspace_bytes == ws
        again = P.transform(XI=XI)
        assert first.tobytes() == want.tobytes() == again.tobytes()
        assert e1.tobytes() == e2.tobytes()
        assert np.array_equal(e3[:, :100], e1[:, :100]) and np.array_equal(e3[:, 100:200], e1[:, 257:357])
        assert P.eval(lam, True).tobytes() == e1.tobytes()      # after another tree run: exported again, same bits
    finally:
        P.close()
        fresh.close()


def test_return_codes(capi, torch):
    L = capi.load()
    import ctypes as C
    x = torch.zeros(64, dtype=torch.complex128, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    Tc, Tbad = (C.c_double * 2)(-2.0, 2.0), (C.c_double * 2)(2.0, 2.0)
    P = EvalPlan(capi, torch, "2SPLIT2_MODAL", 64, 1, 1, 0)
    sub = capi.Plan(64, 0, batch=1, discretization="4SPLIT4B", nskip=2)
    kdv = capi.KdvvPlan(64, 8, batch=1)
    try:
        h = P.plan.h
        # no valid tree run yet
        assert L.fnft_amd_nsev_eval_device(h, Tc, vp(x), 4, 0, 0, vp(x), None) == -FNFT_EC_INVALID_ARGUMENT
        P.transform()
        assert L.fnft_amd_nsev_eval_device(h, None, vp(x), 4, 0, 0, vp(x), None) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft_amd_nsev_eval_device(h, Tc, None, 4, 0, 0, vp(x), None) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft_amd_nsev_eval_device(h, Tc, vp(x), 4, 0, 0, None, None) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft_amd_nsev_eval_device(h, Tbad, vp(x), 4, 0, 0, vp(x), None) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft_amd_nsev_eval_device(h, Tc, vp(x), 4, 3, 0, vp(x), None) == FNFT_EC_INVALID_ARGUMENT
        assert L.fnft_amd_nsev_eval_device(h, Tc, vp(x), 0, 0, 0, vp(x), None) == 0
        assert L.fnft_amd_nsev_eval_device(h, Tc, vp(x), 4, 4, 1, vp(x), None) == 0
        assert P.plan.finish() == 0
        assert L.fnft_amd_nsev_eval_device(kdv.h, Tc, vp(x), 4, 0, 0, vp(x), None) == -FNFT_EC_INVALID_ARGUMENT
        q = dev(torch, PC.nse_signal(64, T, 1, "sub"))
        assert sub.contspec_device(q.data_ptr(), 0, T, (-1.0, 1.0)) == 0 and sub.finish() == 0
        assert L.fnft_amd_nsev_eval_device(sub.h, Tc, vp(x), 4, 0, 0, vp(x), None) == FNFT_EC_NOT_YET_IMPLEMENTED
    finally:
        P.close()
        sub.close()
        kdv.close()


def test_newton_step_on_fast_eigenvalue_roots(capi, torch):
    """The application: 2.2 sech(t) at D = 512 (discspec_batch_cases.signal), the FAST_EIGENVALUE roots of DiscSpecSearchPlan (no refinement: the roots
    of the polynomial a(z) itself), one Newton step lambda - a/a' with the new call's values.

    |a| does not grow at any root whose |a| is above the noise level, and afterwards |a| is at that level at every root
    (the ratios are printed).  The roots come polished to the level, so a step moves them inside the noise and cannot be
    asked to shrink |a| there.  The level: the evaluation's error, at most
    B S with B = max(MARGIN e_dbl, FLOOR_NSE) of the formula run in double at these points; the step lambda - a/a' of
    values that good lands within B S / |a'| of the root, lambda is then rounded (u |lambda|), and the new value carries
    its own B S: |a(lambda_1)| <= 2 B S + u |lambda_1| |a'|."""
    D, Td, disc = 512, DC.T, "2SPLIT2A"
    q = DC.signal(D, 2.2, 0.0)
    K = 8
    search = capi.DiscSpecSearchPlan(D, K, 1, {"discretization": disc, "bound_state_localization": "FAST_EIGENVALUE",
                                               "bound_state_filtering": "FULL", "niter": 0,
                                               "discspec_type": "NORMING_CONSTANTS"})
    P = EvalPlan(capi, torch, disc, D, 1, 1, 0, T=Td, q=q)
    try:
        dbs = torch.zeros(K, dtype=torch.complex128, device="cuda")
        dk = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert search.run_device(P.dq.data_ptr(), list(Td), dbs.data_ptr(), 0, dk.data_ptr()) == 0, capi.last_error()
        rc, st, ko = search.finish()
        assert rc == 0 and st[0] == 0, (rc, st, search.warnings())
        k = int(ko[0])
        lam0 = dbs.cpu().numpy()[:k]
        # i (2.2 - 1/2 - j) of the continuous problem; the scheme's own at eps_t = 0.1 lie O(eps_t^2) away
        assert k == 2 and np.allclose(np.sort(lam0.imag), [0.7, 1.7], atol=5e-2), lam0
        P.transform()
        g0 = P.eval(lam0, True)[0]
        a0, da0 = g0[:k], g0[2 * k:3 * k]
        lam1 = lam0 - a0 / da0
        g1 = P.eval(lam1, True)[0]
        a1 = g1[:k]
        rc, deg, tm, W = P.plan.transfer_matrix(0)
        f = PR.nse_errors(tm, W, lam1, P.consts, g1, True)
        B = PR.bound(f["e_dbl"], PR.FLOOR_NSE)
        assert f["e"] <= B, f
        Sa = f["ref"]["sa"].astype(np.float64)
        level = 2.0 * B * Sa + PR.U * np.abs(lam1) * np.abs(f["ref"]["da"]).astype(np.float64)
        print("lambda", lam1, "|a0|/S", np.abs(a0) / Sa, "|a1|/S", np.abs(a1) / Sa, "level/S", level / Sa,
              "|a1|/level", np.abs(a1) / level, "|a1|/|a0|", np.abs(a1) / np.abs(a0))
        grew = (np.abs(a0) > level) & (np.abs(a1) > np.abs(a0))      # above the noise a step must not make |a| larger
        assert not grew.any(), (np.abs(a0), np.abs(a1), level)
        assert np.all(np.abs(a1) <= level), np.abs(a1) / level
    finally:
        P.close()
        search.close()
