"""The slow-discretization plan (capi.SlowPlan / fnft_amd_slow_plan_*: BO, CF4_2, CF4_3, CF5_3, CF6_4, ES4, TES4) on the
GPU: accuracy against the extended-precision restatement tests/slow_ref.py, the reference's own analytic tests of these
schemes with its bounds, batch and stream semantics, status and warnings, and a cross-check against the
fnft__nse_scatter_matrix seam the parent already had."""
import json
import os

import numpy as np
import pytest

import signals as S
import slow_cases as SC
import slow_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLING = ("CF4_2", "CF4_3", "CF5_3", "CF6_4")


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import build, capi as c
    build.build()
    c.load()
    c.silence_errors()
    return c


@pytest.fixture(scope="module")
def focusing2():
    with open(os.path.join(ROOT, "tests", "golden", "nsev_slow_fixtures.json")) as f:
        return json.load(f)["nsev_sech_focusing2"]


def run_plan(capi, q, T, XI, M, kappa, disc, cstype="BOTH", richardson=0, plan=None):
    """q: (B, D) host array -> (out (B, cs_len) host array, status, warnings)."""
    import torch
    q = np.ascontiguousarray(np.atleast_2d(q), np.complex128)
    own = plan is None
    if own:
        plan = capi.SlowPlan(q.shape[1], M, q.shape[0], {"discretization": disc, "contspec_type": cstype,
                                                         "richardson_extrapolation_flag": richardson})
    try:
        dq = torch.from_numpy(q).cuda()
        out = plan(dq, T, XI, kappa)
        rc, st, wn = plan.finish()
        assert rc == 0, (rc, st)
        assert np.array_equal(dq.cpu().numpy(), q)          # the input is not modified
        return out.cpu().numpy(), st, wn
    finally:
        if own:
            plan.close()


# ---- 1. accuracy against the long-double restatement ---------------------------------------------------------------
# (D, M): two and three samples (both finite-difference ends share a neighbour, one CF group); one lane past a wave with
# odd D through the resampler; one chunk of the plan's rule, the first size with two, three with a ragged last one; the
# last size whose shifts are summed directly and the first that goes through the transform resampler (39, 40); five xi
# tiles (four chunks under the plan's rule)
SHAPES = [(2, 16), (3, 16), (255, 65), (257, 65), (31, 16), (32, 16), (39, 16), (40, 16), (50, 16), (64, 300)]


@pytest.mark.parametrize("kappa", [1, -1])
@pytest.mark.parametrize("disc", SC.DISCS)
def test_accuracy_vs_long_double(capi, disc, kappa):
    """e = max_m |X_gpu - X_ld| / max_m |X_ld| <= 4 e_dbl for rho, a and b, with e_dbl the same figure of the restatement
    run in double (the reference's arithmetic), computed here per case.  D = 2 is not run for the four resampling schemes:
    the reference's resampler rejects it (src/private/fnft__misc.c:331-332) and so does the plan."""
    assert capi.slow_plan_chunks(31, 16)[1] == 1 and capi.slow_plan_chunks(32, 16)[1] == 2
    assert capi.slow_plan_chunks(50, 16) == (17, 3)
    worst = {}
    for D, M in SHAPES:
        if D == 2 and disc in RESAMPLING:
            continue
        out, st, _ = run_plan(capi, SC.signal(D, kappa), SC.interval(kappa), SC.XI, M, kappa, disc)
        assert not st.any()
        e, e_dbl = SC.check("gpu", SC.split_both(out[0], M), disc, kappa, D, M)
        for k in e:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e[k], e_dbl[k]))
    print("largest", disc, kappa, {k: "e=%.2e e_dbl=%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("disc", SC.DISCS)
def test_accuracy_richardson(capi, disc):
    """The Richardson pass (every second sample, combined on the device where |xi| < 0.9 pi / (2 eps_sub)): odd D, two
    chunks in the full pass and one in the second."""
    D, M = 45, 16
    out, st, _ = run_plan(capi, SC.signal(D, 1), SC.interval(1), SC.XI, M, 1, disc, richardson=1)
    assert not st.any()
    SC.check("gpu", SC.split_both(out[0], M), disc, 1, D, M, richardson=1)


# ---- 2. the reference's analytic tests ------------------------------------------------------------------------------
def _slow_files():
    with open(os.path.join(ROOT, "tests", "golden", "reference_fixtures.json")) as f:
        fx = json.load(f)
    files = [b for b in fx["nsev_error_bounds"] if b["discretization"] in SC.DISCS]
    assert len(files) == 14
    return [pytest.param(b, id=b["file"].replace("fnft_nsev_test_", "").replace(".c", "")) for b in files]


def sech_focusing2(D, T):
    t = S.tgrid(T, D)
    return (5.4 * S.sech(t) * np.exp(-6j * t)).astype(np.complex128)


@pytest.mark.parametrize("b", _slow_files())
def test_reference_analytic_bounds(capi, fixtures, focusing2, b):
    """Every harness call of the 14 slow files of the reference's test/fnft_nsev/ -- D, D + 1, D - 1, 2D with the decayed
    bounds and the two Richardson stages -- with the metric of test_fnft_nsev_analytic_bounds (sum |d| / sum |exact|) and
    the file's own first three bounds (rho, a, b), unrelaxed.  The 4th to 6th bounds of each stage belong to the discrete
    spectrum, which the plan does not compute; they are not replayed."""
    if b["testcase"] == "SECH_FOCUSING2":
        fx = focusing2
        sig = lambda D: sech_focusing2(D, fx["T"])  # noqa: E731
        exact = [S.l2c(fx["contspec"]), S.l2c(fx["ab"])[:16], S.l2c(fx["ab"])[16:]]
    else:
        assert b["testcase"] == "SECH_DEFOCUSING"
        fx = fixtures["nsev_sech_defocusing"]
        sig = S.sech_defocusing
        exact = [S.l2c(fx["contspec"])]
    M = fx["M"]
    assert len(b["stages"]) == 6
    for st in b["stages"]:
        out, status, _ = run_plan(capi, sig(st["D"]), fx["T"], fx["XI"], M, fx["kappa"], b["discretization"],
                                  richardson=st["richardson"])
        assert not status.any()
        got = SC.split_both(out[0], M)
        errs = [S.rel_err(got[k], x) for k, x in zip(("rho", "a", "b"), exact)]
        print(b["file"], st["D"], st["richardson"], ["%.2e" % e for e in errs], st["bounds"])
        assert all(np.isfinite(e) for e in errs), (st, errs)
        for e, bound in zip(errs, st["bounds"]):
            if np.isfinite(bound):
                assert e <= bound, (st, errs, b["file"])


# ---- 3. batch semantics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disc", ["BO", "CF5_3", "TES4"])
def test_batch_equals_single_calls_bitwise(capi, disc):
    """Five different signals in one call equal five one-signal calls bit for bit where the chunk count is the same for
    both batch sizes (D = 64, M = 16: four chunks either way)."""
    D, M, B = 64, 16, 5
    assert capi.slow_plan_chunks(D, M, 1) == capi.slow_plan_chunks(D, M, B)
    q = np.stack([SC.signal(D, 1, v) for v in range(B)])
    out, st, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, disc, richardson=1)
    assert not st.any() and out.shape == (B, 3 * M)
    for b in range(B):
        one, _, _ = run_plan(capi, q[b], SC.interval(1), SC.XI, M, 1, disc, richardson=1)
        assert np.array_equal(one[0], out[b]), b


def test_batch_with_another_chunk_count(capi):
    """D = 4096, M = 130: one signal is cut into 256 chunks, each of five into 133, so the product order of a signal differs
    between the two calls.  Both are compared with the long-double restatement at e <= 4 e_dbl instead of bit for bit."""
    D, M, B = 4096, 130, 5
    assert capi.slow_plan_chunks(D, M, 1)[1] != capi.slow_plan_chunks(D, M, B)[1]
    q = np.stack([SC.signal(D, 1, v) for v in range(B)])
    out, st, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, "BO")
    assert not st.any()
    for b in (0, B - 1):
        SC.check("gpu batch=5", SC.split_both(out[b], M), "BO", 1, D, M, variant=b)
        one, _, _ = run_plan(capi, q[b], SC.interval(1), SC.XI, M, 1, "BO")
        SC.check("gpu batch=1", SC.split_both(one[0], M), "BO", 1, D, M, variant=b)


def test_contspec_types_workspace_and_reuse(capi):
    """RHO, AB and BOTH are the same numbers; workspace_bytes > 0; one plan serves another T, XI and kappa."""
    import torch
    D, M = 96, 40
    q = SC.signal(D, 1)
    both, _, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, "CF4_3", "BOTH")
    rho, _, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, "CF4_3", "REFLECTION_COEFFICIENT")
    ab, _, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, "CF4_3", "AB")
    assert rho.shape == (1, M) and ab.shape == (1, 2 * M)
    assert np.array_equal(rho[0], both[0, :M]) and np.array_equal(ab[0], both[0, M:])
    plan = capi.SlowPlan(D, M, 1, {"discretization": "CF4_3", "contspec_type": "BOTH"})
    try:
        assert plan.workspace_bytes > 0
        first, _, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, "CF4_3", plan=plan)
        assert np.array_equal(first, both)
        T2, XI2 = (-2.0, 1.5), (-3.0, 2.0)
        q2 = SC.signal(D, -1)
        other, _, _ = run_plan(capi, q2, T2, XI2, M, -1, "CF4_3", plan=plan)
        fresh, _, _ = run_plan(capi, q2, T2, XI2, M, -1, "CF4_3")
        assert np.array_equal(other, fresh) and not np.array_equal(other, first)
        again, _, _ = run_plan(capi, q, SC.interval(1), SC.XI, M, 1, "CF4_3", plan=plan)
        assert np.array_equal(again, both)
        # errors of the device call: nothing is enqueued
        dq = torch.from_numpy(q[None, :]).cuda()
        dout = torch.zeros((1, 3 * M), dtype=torch.complex128, device="cuda")
        for T, XI, kappa in (((1.0, 1.0), SC.XI, 1), ((2.0, 1.0), SC.XI, 1), (SC.T_FOC, (1.0, 1.0), 1),
                             (SC.T_FOC, (2.0, -2.0), 1), (SC.T_FOC, SC.XI, 0), (SC.T_FOC, SC.XI, 2)):
            assert plan.run_device(dq.data_ptr(), T, XI, dout.data_ptr(), kappa) == capi.FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(0, SC.T_FOC, SC.XI, dout.data_ptr(), 1) == capi.FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(dq.data_ptr(), SC.T_FOC, SC.XI, 0, 1) == capi.FNFT_EC_INVALID_ARGUMENT
        assert not dout.cpu().numpy().any()
    finally:
        plan.close()


def test_two_streams_two_plans(capi):
    """Two calls on two streams with two plans match their serial results."""
    import torch
    D, M, B = 512, 64, 3
    qa = np.stack([SC.signal(D, 1, v) for v in range(B)])
    qb = np.stack([SC.signal(D, -1, v) for v in range(B)])
    ra, _, _ = run_plan(capi, qa, SC.interval(1), SC.XI, M, 1, "CF6_4")
    rb, _, _ = run_plan(capi, qb, SC.interval(-1), SC.XI, M, -1, "ES4")
    pa = capi.SlowPlan(D, M, B, {"discretization": "CF6_4", "contspec_type": "BOTH"})
    pb = capi.SlowPlan(D, M, B, {"discretization": "ES4", "contspec_type": "BOTH"})
    try:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        da, db = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
        torch.cuda.synchronize()
        oa = pa(da, SC.interval(1), SC.XI, 1, stream=sa)
        ob = pb(db, SC.interval(-1), SC.XI, -1, stream=sb)
        assert pa.finish()[0] == 0 and pb.finish()[0] == 0
        assert np.array_equal(oa.cpu().numpy(), ra) and np.array_equal(ob.cpu().numpy(), rb)
    finally:
        pa.close()
        pb.close()


def test_one_signal_convenience(capi):
    D, M = 40, 16
    rc, cs, warn = capi.nsev_slow(SC.signal(D, 1), SC.interval(1), M, SC.XI, 1, "ES4", "BOTH")
    assert rc == 0 and warn == 0
    SC.check("gpu nsev_slow", SC.split_both(cs, M), "ES4", 1, D, M)


# ---- 4. status and warnings -----------------------------------------------------------------------------------------
def test_not_bandlimited_warning_per_signal(capi):
    """The rectangular pulse of test_not_bandlimited_warning sets bit 0 of its own warnings slot under CF4_3 (the
    resampler's finding, src/private/fnft__misc.c:371-381), the smooth pulse next to it does not, and BO -- no
    resampling -- never does.

    No DIV_BY_ZERO case: the fast plan's test zeroes the a-polynomial of a caller-supplied transfer matrix; a slow scheme
    has no such input, and a(xi) of a product of matrix exponentials is exactly 0 only if cos and sin values of the
    device's own functions cancel to the last bit, which no signal can be constructed to guarantee.  The status path is
    the same atomic-or the fast plan uses."""
    D, M = 1024, 32
    T, XI = [-25.0, 25.0], [-1.4, 1.6]
    rect = np.where(np.abs(S.tgrid(T, D)) < 3.0, 1.5 + 0j, 0j)
    q = np.stack([S.sech_focusing(D), rect, S.sech_focusing(D, amp=1.0)])
    _, st, wn = run_plan(capi, q, T, XI, M, 1, "CF4_3")
    assert not st.any() and list(wn) == [0, 1, 0]
    _, st, wn = run_plan(capi, q, T, XI, M, 1, "BO")
    assert not st.any() and not wn.any()


# ---- 5. cross-check against the scatterer seam of the parent ---------------------------------------------------------
@pytest.mark.parametrize("disc", ["BO", "CF4_2"])
def test_matches_scatter_matrix_seam(capi, disc):
    """a and b of the plan against fnft__nse_scatter_matrix (chunk-parallel over the samples, pinned by the reference's
    BO vector) at the same preprocessed samples and xi after the same phase factors; bound as in the accuracy test."""
    D, M, kappa = 200, 48, 1
    q, T = SC.signal(D, kappa), SC.interval(kappa)
    eps_t = (T[1] - T[0]) / (D - 1)
    xi = SC.XI[0] + (SC.XI[1] - SC.XI[0]) / (M - 1) * np.arange(M)
    if disc == "BO":
        qp = q
    else:
        s = np.sqrt(3.0) / 6.0
        rc1, q1 = capi.misc_resample(q, eps_t, -eps_t * s)
        rc2, q2 = capi.misc_resample(q, eps_t, eps_t * s)
        assert rc1 == 0 and rc2 == 0
        qp = np.empty(2 * D, np.complex128)
        qp[0::2] = (0.25 + s) * q1 + (0.25 - s) * q2
        qp[1::2] = (0.25 - s) * q1 + (0.25 + s) * q2
    rc, sm = capi.nse_scatter_matrix(qp, eps_t, kappa, xi.astype(np.complex128), derivative=False, discretization=disc)
    assert rc == 0
    a_seam = sm[:, 0] * np.exp(1j * xi * ((T[1] + eps_t * 0.5) - (T[0] - eps_t * 0.5)))
    b_seam = sm[:, 2] * np.exp(1j * xi * (-(T[1] + eps_t * 0.5) - (T[0] - eps_t * 0.5)))
    out, _, _ = run_plan(capi, q, T, SC.XI, M, kappa, disc, "AB")
    _, e_dbl = SC.reference(disc, kappa, D, M)
    for name, got, ref in (("a", out[0, :M], a_seam), ("b", out[0, M:], b_seam)):
        e = SR.rel_max(got, ref)
        print(disc, name, "plan vs seam e=%.2e  e_dbl=%.2e" % (e, e_dbl[name]))
        assert e <= SC.MARGIN * e_dbl[name]
