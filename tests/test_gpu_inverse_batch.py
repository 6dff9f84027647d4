"""The batched, device-resident inverse (capi.InversePlan: fnft_amd_inverse_plan_create / fnft_amd_nsev_inverse_device
/ fnft_amd_inverse_plan_finish) on the GPU: run-time argument codes, per-slot agreement with the drop-in
fnft_nsev_inverse on every admissible option set, independence of the slots, the reference's error bounds, a device
round trip from the batched forward plan, per-signal status and warnings, and a larger size."""

import numpy as np
import pytest

import inverse_cases as IC
import signals as S

pytestmark = pytest.mark.gpu
DISCS = ("2SPLIT2A", "2SPLIT2_MODAL")
T_STD = [-8.0, 8.0]


@pytest.fixture(scope="module")
def capi():
    from fnft_amd import capi as c
    c.load()
    c.silence_errors()
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def run_batch(capi, torch, D, M, opts, cs_rows, XI, T, kappa, stream=None):
    """One call of the batched inverse on the rows of cs_rows: (rc, q[B, D], status[B], warnings[B])."""
    cs = np.ascontiguousarray(np.stack(cs_rows), np.complex128)
    B = cs.shape[0]
    plan = capi.InversePlan(D, M, B, opts)
    try:
        dcs = torch.from_numpy(cs.reshape(-1)).to("cuda")
        dq = torch.full((B * D,), complex("nan"), dtype=torch.complex128, device="cuda")
        sp = 0 if stream is None else stream.cuda_stream
        torch.cuda.synchronize()
        rc = plan.run_device(dcs.data_ptr(), dq.data_ptr(), XI, T, kappa, sp)
        assert rc == 0, (rc, capi.last_error())
        rcf, st, wn = plan.finish(sp)
        q = dq.cpu().numpy().reshape(B, D)
        # the contspec is not modified
        assert np.array_equal(dcs.cpu().numpy().reshape(B, M), cs)
    finally:
        plan.close()
    return rcf, q, st, wn


def signals(D, T=T_STD, seed=0):
    """Five different pulses: sech pulses below the soliton threshold with different amplitude and chirp, a truncated
    soliton and a smooth random pulse."""
    t = S.tgrid(T, D)
    rng = np.random.default_rng(seed + D)
    c = rng.standard_normal(6) + 1j * rng.standard_normal(6)
    smooth = np.exp(-(t / 2.5) ** 2) * sum(c[k] * np.exp(1j * k * t / 3.0) for k in range(6)) * 0.05
    return [0.3 * IC.sech(t),
            0.45 * IC.sech(t) * np.exp(-0.15j * t * t),
            0.25 * IC.sech(1.5 * (t - 1.0)) * np.exp(0.1j * t * t),
            np.where(t <= 0, IC.sech(t), 0.0) + 0j,
            smooth]


_fwd = {}


def spectra(capi, D, M, disc, kappa, cstype):
    """Inputs of the batched call: forward spectra of signals() (capi.fnft_nsev), rho or b(xi), and the grid XI."""
    key = (D, M, disc, kappa)
    if key not in _fwd:
        rc, XI = capi.nsev_inverse_XI(D, T_STD, M, disc)
        assert rc == 0
        rows = []
        for q in signals(D):
            rc, cs = capi.fnft_nsev(q, T_STD, M, XI, kappa=kappa, discretization=disc, contspec_type="BOTH")
            assert rc == 0, capi.last_error()
            rows.append((cs[:M].copy(), cs[2 * M:3 * M].copy()))
        _fwd[key] = (XI, rows)
    XI, rows = _fwd[key]
    return XI, [r[0] if cstype == "REFLECTION_COEFFICIENT" else r[1] for r in rows]


def b_of_tau_rows(D, T=(-25.0, 25.0)):
    """B(tau) of sech pulses of different amplitude and position (the B_of_tau cases of inverse_cases.py)."""
    t = S.tgrid(T, D)
    return [1j / (2 * np.pi) * np.sin(np.pi * A) * IC.sech((2 * t - 2 * t0) / 2)
            for A, t0 in ((0.45, 1.2), (0.3, 0.0), (0.2, -2.0), (0.4, 3.0), (0.35, -0.5))]


def drop_in(capi, M, cs, XI, D, T, kappa, opts):
    return capi.fnft_nsev_inverse(M, np.array(cs, np.complex128), XI, None, None, D, list(T), kappa, opts)


def assert_slot_equal(q, ref, tol=1e-13):
    scale = np.max(np.abs(ref))
    d = np.max(np.abs(q - ref))
    assert d <= tol * max(scale, 1e-300), (d, scale)


# ---- 0. run-time argument checks ----------------------------------------------------------------------------------
def test_run_time_argument_codes_follow_the_drop_in(capi, torch):
    D, M, T = 8, 16, [0.0, 7.0]
    rc, XI = capi.nsev_inverse_XI(D, T, M)
    cs = torch.full((M,), 0.01, dtype=torch.complex128, device="cuda")
    q = torch.zeros(D, dtype=torch.complex128, device="cuda")
    csn = np.full(M, 0.01 + 0j)

    def both(plan_opts, Mp, T_, kappa, XI_):
        p = capi.InversePlan(D, Mp, 1, plan_opts)
        try:
            r = p.run_device(cs.data_ptr(), q.data_ptr(), XI_, T_, kappa)
        finally:
            p.close()
        r0, _ = capi.fnft_nsev_inverse(Mp, csn[:Mp].copy(), XI_, None, None, D, T_, kappa, plan_opts)
        return r, r0

    for args, code in ((({}, M, [7.0, 0.0], 1, XI), 2), (({}, M, T, 0, XI), 2), (({}, M, T, 1, None), 2),
                       (({"contspec_type": "B_OF_XI"}, M, T, -1, None), 2),
                       (({"contspec_type": "B_OF_TAU"}, D, T, 1, None), -2)):
        r, r0 = both(*args)
        assert r == r0 == code, (args, r, r0)


# ---- 1. parity with the drop-in -------------------------------------------------------------------------------------
CONFIGS = [("REFLECTION_COEFFICIENT", m) for m in ("DEFAULT", "TFMATRIX_CONTAINS_REFL_COEFF")] + \
          [("B_OF_XI", "DEFAULT"), ("B_OF_TAU", "DEFAULT")]


@pytest.mark.parametrize("D", (2, 4, 256, 1024, 4096))
@pytest.mark.parametrize("kappa", (1, -1))
@pytest.mark.parametrize("disc", DISCS)
@pytest.mark.parametrize("cstype, method", CONFIGS)
def test_every_slot_equals_the_drop_in(capi, torch, cstype, method, disc, kappa, D):
    opts = {"discretization": disc, "contspec_type": cstype, "contspec_inversion_method": method}
    if cstype == "B_OF_TAU":
        cases = [(D, [-25.0, 25.0], None, b_of_tau_rows(D))]
    else:
        cases = []
        for M in (D, 2 * D):
            XI, rows = spectra(capi, D, M, disc, kappa, cstype)
            cases.append((M, T_STD, XI, rows))
    for M, T, XI, rows in cases:
        rc, q, st, wn = run_batch(capi, torch, D, M, opts, rows, XI, T, kappa)
        for b, cs in enumerate(rows):
            r0, q0 = drop_in(capi, M, cs, XI, D, T, kappa, opts)
            assert st[b] == r0, (M, b, st[b], r0)
            if r0 == 0:
                assert_slot_equal(q[b], q0)
        assert rc == next((int(s) for s in st if s != 0), 0)


@pytest.mark.parametrize("D", (8192, 16384))
@pytest.mark.parametrize("disc, kappa", (("2SPLIT2_MODAL", 1), ("2SPLIT2A", -1)))
def test_every_slot_equals_the_drop_in_where_step_4_is_a_plan(capi, torch, disc, kappa, D):
    """The sizes above reach every one-launch product of the layer peeling but no product of the inverses (step 4)
    through a plan: D = 8192 is the first with one (degree 2048), D = 16384 the first at degree 4096 -- here with the
    batch strides of T, Ti and the product's output (tests/peel_cases.py, PATHS)."""
    opts = {"discretization": disc, "contspec_type": "B_OF_XI", "contspec_inversion_method": "DEFAULT"}
    XI, rows = spectra(capi, D, D, disc, kappa, "B_OF_XI")
    rc, q, st, wn = run_batch(capi, torch, D, D, opts, rows, XI, T_STD, kappa)
    for b, cs in enumerate(rows):
        r0, q0 = drop_in(capi, D, cs, XI, D, T_STD, kappa, opts)
        assert st[b] == r0 == 0, (b, st[b], r0)      # every slot is compared
        assert_slot_equal(q[b], q0)
    assert rc == 0


# ---- 2. independence of the slots -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cstype", ("REFLECTION_COEFFICIENT", "B_OF_XI"))
def test_slots_are_independent(capi, torch, cstype):
    D, M, disc, kappa = 4096, 8192, "2SPLIT2_MODAL", 1
    opts = {"discretization": disc, "contspec_type": cstype}
    XI, rows = spectra(capi, D, M, disc, kappa, cstype)
    rows7 = rows + [0.5 * rows[0], 0.7 * rows[4]]
    _, q7, st7, _ = run_batch(capi, torch, D, M, opts, rows7, XI, T_STD, kappa)
    assert (st7 == 0).all()
    perm = [3, 6, 0, 5, 1, 4, 2]
    _, qp, _, _ = run_batch(capi, torch, D, M, opts, [rows7[i] for i in perm], XI, T_STD, kappa)
    assert np.array_equal(qp, q7[perm])
    for b in (0, 4):
        _, q1, _, _ = run_batch(capi, torch, D, M, opts, [rows7[b]], XI, T_STD, kappa)
        assert np.array_equal(q1[0], q7[b])


# ---- 3. the reference's bounds --------------------------------------------------------------------------------------
def bound_case_batch(capi, torch, case):
    """The case in the middle slot of a batch of three (the outer slots: the same spectrum at half the amplitude)."""
    cs = np.array(case["contspec"], np.complex128)
    o = dict(case["opts"])
    rc, q, st, _ = run_batch(capi, torch, case["D"], case["M"], o, [0.5 * cs, cs, 0.5 * cs], case.get("XI"), case["T"],
                             case["kappa"])
    assert rc == 0 and (st == 0).all(), (rc, st)
    err = S.rel_err(q[1], case["q_exact"])
    assert err < case["bound"], (err, case["bound"])
    assert np.array_equal(q[0], q[2])


def _xi_of(capi):
    return lambda D, T, M: capi.nsev_inverse_XI(D, T, M)[1]


@pytest.mark.parametrize("n", (2048, 4096))
@pytest.mark.parametrize("tag", ("2split2A", "2split2_modal"))
def test_sech_defocusing_meets_the_reference_bound(capi, torch, tag, n):
    bound_case_batch(capi, torch, IC.sech_defocusing(tag, n))


@pytest.mark.parametrize("step", range(4))
@pytest.mark.parametrize("tag", ("2split2A", "2split2_modal"))
@pytest.mark.parametrize("kind", ("B_of_tau", "b_of_xi"))
def test_b_cases_meet_the_reference_bound(capi, torch, kind, tag, step):
    bound_case_batch(capi, torch, IC.b_cases(kind, False, tag, step, _xi_of(capi)))


# ---- 4. device round trip -------------------------------------------------------------------------------------------
def test_device_round_trip_64_signals(capi, torch):
    """64 signals of D = 4096: batched forward plan (rho, M = 2D) then the batched inverse on a non-default stream,
    nothing on the host in between; the bound of test_full_size_round_trip."""
    D, B, M, T, disc = 4096, 64, 8192, [-32.0, 32.0], "2SPLIT2_MODAL"
    t = S.tgrid(T, D)
    rng = np.random.default_rng(7)
    amp, t0, f = rng.uniform(0.2, 0.4, B), rng.uniform(-2, 2, B), rng.uniform(-1, 1, B)
    q0 = np.stack([a / np.cosh(t - s) * np.exp(-1j * w * t) for a, s, w in zip(amp, t0, f)])
    rc, XI = capi.nsev_inverse_XI(D, T, M, disc)
    assert rc == 0
    fwd = capi.Plan(D, M, B, disc)
    inv = capi.InversePlan(D, M, B, {"discretization": disc})
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            dq0 = torch.from_numpy(q0.reshape(-1)).to("cuda", non_blocking=False)
            dcs = torch.empty(B * M, dtype=torch.complex128, device="cuda")
            dq = torch.empty(B * D, dtype=torch.complex128, device="cuda")
        stream.synchronize()
        sp = stream.cuda_stream
        assert fwd.contspec_device(dq0.data_ptr(), dcs.data_ptr(), T, XI, 1, "REFLECTION_COEFFICIENT", stream=sp) == 0
        assert inv.run_device(dcs.data_ptr(), dq.data_ptr(), XI, T, 1, sp) == 0
        assert fwd.finish(sp) == 0
        rc, st, wn = inv.finish(sp)
        assert rc == 0 and (st == 0).all() and (wn == 0).all()
        q = dq.cpu().numpy().reshape(B, D)
    finally:
        inv.close()
        fwd.close()
    errs = [S.rel_err(q[b], q0[b]) for b in range(B)]
    assert max(errs) < 1e-5, max(errs)


# ---- 5. per-signal status -------------------------------------------------------------------------------------------
class WarningCounter:
    def __init__(self, capi):
        self.capi = capi
        self.n = 0

        def cb(fmt):
            if fmt and fmt.startswith(b"FNFT Warning"):
                self.n += 1
            return 0
        self.cb = capi.PRINTF_T(cb)

    def __enter__(self):
        self.capi.load().fnft_errwarn_setprintf(self.cb)
        return self

    def __exit__(self, *a):
        self.capi.silence_errors()


@pytest.mark.parametrize("kappa", (-1, 1))
def test_ill_posed_slot_is_reported_alone(capi, torch, kappa):
    """One B_OF_XI slot with |b(xi)| > 1 on part of the grid.  The drop-in flags the spectral factorization as
    ill-posed only where 1 - kappa'|b|^2 nearly vanishes (the focusing branch); defocusing it goes through without a
    warning.  Either way the slot's status and warning equal the drop-in's, and the other slots are bitwise those of a
    batch without it."""
    D, M, disc = 1024, 2048, "2SPLIT2A"
    opts = {"discretization": disc, "contspec_type": "B_OF_XI"}
    XI, rows = spectra(capi, D, M, disc, kappa, "B_OF_XI")
    big = rows[1] * (1.5 / np.max(np.abs(rows[1])))
    assert np.max(np.abs(big)) > 1.0
    with WarningCounter(capi) as w:
        r0, _ = drop_in(capi, M, big, XI, D, T_STD, kappa, opts)
    warned = 1 if w.n else 0
    if kappa == 1:
        assert warned == 1
    batch = [rows[0], big, rows[2], rows[3]]
    rc, q, st, wn = run_batch(capi, torch, D, M, opts, batch, XI, T_STD, kappa)
    assert st[1] == r0 and wn[1] == warned
    assert (np.delete(st, 1) == 0).all() and (np.delete(wn, 1) == 0).all()
    assert rc == r0
    _, q3, _, _ = run_batch(capi, torch, D, M, opts, [rows[0], rows[2], rows[3]], XI, T_STD, kappa)
    assert np.array_equal(np.delete(q, 1, axis=0), q3)


# ---- 6. larger size -------------------------------------------------------------------------------------------------
def test_b_of_xi_batch_of_8_at_2p16(capi, torch):
    D, M, disc, kappa = 1 << 16, 1 << 16, "2SPLIT2_MODAL", 1
    T = [-32.0, 32.0]
    rc, XI = capi.nsev_inverse_XI(D, T, M, disc)
    xi = XI[0] + (XI[1] - XI[0]) / (M - 1) * np.arange(M)
    rows = [1j * np.exp(-2j * xi * t0) * np.sin(np.pi * A) / np.cosh(np.pi * xi)
            for A, t0 in zip(np.linspace(0.1, 0.45, 8), np.linspace(-3, 3, 8))]
    opts = {"discretization": disc, "contspec_type": "B_OF_XI"}
    rc, q, st, _ = run_batch(capi, torch, D, M, opts, rows, XI, T, kappa)
    assert rc == 0 and (st == 0).all()
    for b, cs in enumerate(rows):
        r0, q0 = drop_in(capi, M, cs, XI, D, T, kappa, opts)
        assert r0 == 0
        assert_slot_equal(q[b], q0)
