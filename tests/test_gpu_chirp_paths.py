"""Every chirp z-transform path on the GPU against the extended-precision reference (tests/chirp_ref.py).

Each case of tests/chirp_cases.py runs through its entry point (rc 0); the values at K output indices are compared
with the reference, mass-relative, against the bound of the case's form.  The polynomials of the epilogue cases are
the plans' own transfer matrices (fnft_amd_plan_get_transfer_matrix, for the KdV plan on its handle too): they are
bitwise the coefficients the chirp reads (the export and the chirp's coefficient load form the same stored value times
the same scale), so the comparison isolates the chirp and its epilogue from the tree.  Plan and KdV plan cases also
check the launched kernels against the case's list."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import chirp_cases as CC
import chirp_ref as R

pytestmark = pytest.mark.gpu

_measured = {}


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    c.silence_errors()
    yield c
    out = os.environ.get("FNFT_CHIRP_ERR_JSON")   # optional record of the measured errors
    if out:
        with open(out, "w") as f:
            json.dump(_measured, f, indent=1)


def _check(key, e, L, Phi, Cb):
    b = R.err_bound(Cb, L, Phi)
    _measured[key] = dict(e=e, bound=b, e_over_u_log2L=e / R.err_bound((1.0, 0.0), L), Phi=Phi,
                          e_over_u_Phi=(e / (R.U * Phi)) if Phi > 0 else None)
    assert e < b, (key, e, b)


def _full_name(n):
    """The launch timers print __PRETTY_FUNCTION__'s K, which leaves out template arguments equal to their defaults
    (KChirpColFwd<N1> for KChirpColFwd<N1,false>): spell them out as the emulator's demangled names do."""
    n = n.replace(" ", "")
    for k, defaults in (("KChirpColFwd<", ["false"]), ("KChirpColInv<", ["false", "false"])):
        if n.startswith(k):
            args = n[len(k):-1].split(",")
            return k + ",".join(args + defaults[len(args) - 1:]) + ">"
    return n


def _names(plan):
    return [_full_name(n) for n, _ in plan.launch_times()]


def _check_names(c, names):
    missing = [k for k in CC.kernels(c) if k not in names]
    assert not missing, (missing, names)
    unwanted = [k for k in c["absent"] if k in names]
    assert not unwanted, (unwanted, names)


def _tm(capi, h, b, numel):
    """Transfer matrix b of a plan handle (Plan or KdvvPlan) through fnft_amd_plan_get_transfer_matrix."""
    L = capi.load()
    buf = np.zeros(numel, np.complex128)
    deg = C.c_size_t(0)
    W = C.c_int32(0)
    rc = L.fnft_amd_plan_get_transfer_matrix(h, b, buf.ctypes.data_as(C.c_void_p), C.byref(deg), C.byref(W))
    assert rc == 0, capi.last_error()
    d = deg.value
    return buf[: 4 * (d + 1)].reshape(4, d + 1).copy(), int(W.value)


def _nse_check(c, key, out, tm, W, T, XI, M, D, deg1, cstype, L):
    """Compare one signal's contspec output (rho / a, b in the fnft_nsev layout) with the reference."""
    shifted = c["disc"] in ("2SPLIT2_MODAL", "2SPLIT2A")
    m = CC.out_points(c, M)
    ref = R.nsev_epilogue_ref(tm, W, T, XI, M, D, deg1, shifted, m)
    Phi = R.phi(L, *R.nsev_grid(T, XI, M, D, deg1)) + ref["phi_pf"]
    off = 0
    if cstype in ("REFLECTION_COEFFICIENT", "BOTH"):
        _check(key + "[rho]", R.quotient_error(out[m], ref["rho"], ref["H11"], ref["mass"]), L, Phi, CC.BOUND_NSE)
        off = M
    if cstype in ("AB", "BOTH"):
        sm = ref["mass"] * ref["scale"]
        _check(key + "[a]", R.error(out[off + m], ref["a"], sm), L, Phi, CC.BOUND_NSE)
        _check(key + "[b]", R.error(out[off + M + m], ref["b"], sm), L, Phi, CC.BOUND_NSE)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_ids())
def test_chirp_path(capi, oracle, case):
    import torch
    c = case
    L = CC.ROW * c["N1"]
    if c["entry"] == "chirpz":
        p, A, W, m0 = CC.chirpz_inputs(c)
        rc, x = capi.poly_chirpz(p, A, W, c["M"])
        assert rc == 0, capi.last_error()
        m = CC.out_points(c, c["M"], [m0])
        ref, mass = R.chirpz_ref(p, A, W, m)
        _check(c["id"], R.error(x[m], ref, mass), L, R.phi(L, A, W), CC.BOUND_RAW)
        return
    if c["entry"] == "resample":
        q, eps_t, delta = CC.resample_inputs(c)
        rc, qn = capi.misc_resample(q, eps_t, delta)
        assert rc == 0, capi.last_error()
        j = CC.out_points(c, q.size)
        mass = R.resample_mass(q)
        _check(c["id"], R.error(qn[j], R.resample_ref(q, eps_t, delta, j), mass), L, 0.0, CC.BOUND_DFT)
        # every output point against the oracle (a wrong tile of columns that K points can miss)
        rc, qo = oracle.misc_resample(q, eps_t, delta)
        assert rc == 0
        _check(c["id"] + "[oracle]", float(np.max(np.abs(qn - qo))) / mass, L, 0.0, CC.BOUND_DFT)
        return
    B, D, M = c["batch"], c["D"], c["M"]
    T, XI = CC.grid(c)
    deg1 = CC.DEG0[c["disc"]]
    if c["entry"] == "kdv":
        us = CC.kdv_signals(c, T)
        plan = capi.KdvvPlan(D, M, batch=B, discretization=c["disc"])
        assert plan.set_real_mode(c["real"]) == 0
        du = torch.from_numpy(np.concatenate(us)).cuda()
        out = torch.zeros(B * M, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        plan.set_launch_timing(True)
        rc = plan.contspec_device(du.data_ptr(), out.data_ptr(), T, XI)
        assert rc == 0, capi.last_error()
        assert plan.finish() == 0
        _check_names(c, _names(plan))
        res = out.cpu().numpy()
        numel = 4 * (D * deg1 + 1)
        for b in range(B):
            tm, _ = _tm(capi, plan.h, b, numel)
            m = CC.out_points(c, M)
            ref = R.kdvv_epilogue_ref(tm, T, XI, M, D, deg1, c["disc"] == "2SPLIT2A", m)
            Phi = R.phi(L, *R.kdvv_grid(T, XI, M, D, deg1)) + ref["phi_pf"]
            e = R.quotient_error(res[b * M + m], ref["rho"], ref["den"], ref["mass"])
            _check("%s[b=%d]" % (c["id"], b), e, L, Phi, CC.BOUND_KDV)
        plan.close()
        return
    cs = c["cstype"]
    plan = capi.Plan(D, M, batch=B, discretization=c["disc"])
    cl = plan.cs_len(cs)
    out = torch.zeros(B * cl, dtype=torch.complex128, device="cuda")
    numel = 4 * (D * deg1 + 1)
    if c["entry"] == "tm":
        tms = CC.tm_inputs(c)
        dtm = torch.from_numpy(tms.reshape(-1)).cuda()
        torch.cuda.synchronize()
        plan.set_launch_timing(True)
        rc = plan.contspec_from_tm_device(dtm.data_ptr(), c["W"], out.data_ptr(), T, XI, contspec_type=cs)
        assert rc == 0, capi.last_error()
        assert plan.finish() == 0
        _check_names(c, _names(plan))
        res = out.cpu().numpy()
        for b in range(B):
            _nse_check(c, "%s[b=%d]" % (c["id"], b), res[b * cl:(b + 1) * cl], tms[b], c["W"], T, XI, M, D, deg1,
                       cs, L)
        plan.close()
        return

    def run(pl, sig, XIr):
        dq = torch.from_numpy(np.concatenate(sig)).cuda()
        o = torch.zeros(B * cl, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        rc = pl.contspec_device(dq.data_ptr(), o.data_ptr(), T, XIr, kappa=c.get("kappa", 1), contspec_type=cs)
        assert rc == 0, capi.last_error()
        assert pl.finish() == 0
        return o.cpu().numpy()

    def compare(pl, res, XIr, tag):
        for b in range(B):
            tm, W = _tm(capi, pl.h, b, numel)
            _nse_check(c, "%s%s[b=%d]" % (c["id"], tag, b), res[b * cl:(b + 1) * cl], tm, W, T, XIr, M, D, deg1, cs, L)

    s0 = CC.nse_signals(c, T)
    plan.set_launch_timing(True)
    r0 = run(plan, s0, XI)
    _check_names(c, _names(plan))
    compare(plan, r0, XI, "")
    if c["entry"] == "cache":
        # same grid, another signal: the filter spectrum is reloaded (v_mode 2) -- bitwise what a fresh plan computes
        s1 = CC.nse_signals(c, T, salt=1)
        r1 = run(plan, s1, XI)
        fresh = capi.Plan(D, M, batch=B, discretization=c["disc"])
        rf = run(fresh, s1, XI)
        fresh.close()
        assert np.array_equal(r1.view(np.float64), rf.view(np.float64))
        # XI shifted by an exact binary step: same V (cache hit), another A; then another width (key miss)
        XIs = (XI[0] + 0.125, XI[1] + 0.125)
        assert (XIs[1] - XIs[0]) == (XI[1] - XI[0])
        compare(plan, run(plan, s1, XIs), XIs, "[shift]")
        XIw = (XI[0], XI[0] + 1.5 * (XI[1] - XI[0]))
        compare(plan, run(plan, s0, XIw), XIw, "[wide]")
    plan.close()
