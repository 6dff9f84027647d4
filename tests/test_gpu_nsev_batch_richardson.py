"""Richardson extrapolation on the batched tree plan (capi.Plan.set_richardson: fnft_amd_plan_set_richardson) on the GPU:
every slot against the oracle and against the drop-in fnft_nsev with richardson_extrapolation_flag = 1 on that signal
alone, the mask of extrapolated grid points, the setter's behaviour as a switch, the status of the coarse pass and the
setter's error codes."""
import numpy as np
import pytest

import signals as S
from richardson_cases import CS_CASES, CS_M, CS_T, CS_TYPES, CS_XI, cs_signals

pytestmark = pytest.mark.gpu
T, XI, M = [-25.0, 25.0], [-1.4, 1.6], 64
CASES = [("2SPLIT4A", 1, 1024), ("2SPLIT4A", -1, 1025), ("2SPLIT2A", 1, 751), ("2SPLIT2_MODAL", 1, 1000),
         ("4SPLIT4A", 1, 512), ("4SPLIT4B", -1, 400), ("4SPLIT4A", 1, 511)]
AMPS = {1: (3.2, 2.3, 1.4), -1: (1.1, 0.8, 0.5)}
TYPES = [("BOTH", "BOTH", 3), ("AB", "AB", 2), ("REFLECTION_COEFFICIENT", "RHO", 1)]      # capi name, oracle name, parts
ORACLE_REL = 1e-11          # per part, test_gpu_parity.py: test_fnft_nsev_richardson_vs_oracle
# Comparison with the drop-in: the same kernels on the same grids, combined by the same formula in the same order of
# operations -- on the host there, in KRichCombineCs here.  Largest relative L1 disagreement per part measured on an
# MI355X over every comparison with the drop-in in this file (each prints its figure): 0.000e+00, every value agrees bit
# for bit.  The bound is 10x that, i.e. equality, and never above the oracle bound.
DROPIN_MEASURED = 0.0
DROPIN_REL = min(10 * DROPIN_MEASURED, ORACLE_REL)


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


def signals(kappa, D):
    return np.stack([S.sech_focusing(D, T, amp=a) for a in AMPS[kappa]])


def run(capi, torch, plan, q, cst, kappa=1, Tq=T, XIq=XI, calls=1):
    """`calls` contspec_device calls on `plan`: (rc of finish, contspec[B, parts, M] of the last call); back-to-back
    calls must agree bitwise and leave the workspace as it is."""
    B = q.shape[0]
    n = plan.cs_len(cst)
    dq = torch.from_numpy(np.ascontiguousarray(q).reshape(-1)).to("cuda")
    ws = plan.workspace_bytes
    outs = []
    for _ in range(calls):
        out = torch.zeros(B * n, dtype=torch.complex128, device="cuda")
        rc = plan.contspec_device(dq.data_ptr(), out.data_ptr(), list(Tq), list(XIq), kappa=kappa, contspec_type=cst)
        assert rc == 0, (rc, capi.last_error())
        outs.append(out)
    rcf = plan.finish()
    assert plan.workspace_bytes == ws
    assert np.array_equal(dq.cpu().numpy().reshape(q.shape), q)
    res = [o.cpu().numpy().reshape(B, n // plan.M, plan.M) for o in outs]
    for r in res[1:]:
        assert np.array_equal(r, res[0], equal_nan=True)
    return rcf, res[0]


_RUNS = {}


def batched(capi, torch, disc, kappa, D):
    """{capi type name: contspec[3, parts, M]} of one of CASES with the setter on, computed once."""
    key = (disc, kappa, D)
    if key not in _RUNS:
        plan = capi.Plan(D, M, 3, disc)
        try:
            assert plan.set_richardson(True) == 0
            q = signals(kappa, D)
            out = {}
            for cname, _, _ in TYPES:
                rcf, out[cname] = run(capi, torch, plan, q, cname, kappa)
                assert rcf == 0
            _RUNS[key] = out
        finally:
            plan.close()
    return _RUNS[key]


@pytest.mark.parametrize("disc,kappa,D", CASES)
def test_against_the_oracle(capi, torch, oracle, disc, kappa, D):
    got = batched(capi, torch, disc, kappa, D)
    q = signals(kappa, D)
    worst = 0.0
    for cname, oname, parts in TYPES:
        for b in range(3):
            rc, ref = oracle.fnft_nsev(q[b], T, M, XI, kappa=kappa, disc=disc, cstype=oname, richardson=True)
            assert rc == 0
            ref = ref.reshape(parts, M)
            for j in range(parts):
                e = S.rel_err(got[cname][b, j], ref[j])
                worst = max(worst, e)
                assert e < ORACLE_REL, (cname, b, j, e)
    print("vs oracle %s kappa %d D=%d: %.3e" % (disc, kappa, D, worst))


WORST = {"cs": 0.0}


@pytest.mark.parametrize("disc,kappa,D", CASES)
def test_against_the_drop_in(capi, torch, disc, kappa, D):
    got = batched(capi, torch, disc, kappa, D)
    q = signals(kappa, D)
    worst = 0.0
    for cname, _, parts in TYPES:
        for b in range(3):
            rc, cs = capi.fnft_nsev(q[b], T, M, XI, kappa=kappa, discretization=disc, contspec_type=cname, richardson=True)
            assert rc == 0, capi.last_error()
            cs = cs.reshape(parts, M)
            for j in range(parts):
                worst = max(worst, S.rel_err(got[cname][b, j], cs[j]))
    WORST["cs"] = max(WORST["cs"], worst)
    print("vs drop-in %s kappa %d D=%d: %.3e; worst so far %.3e" % (disc, kappa, D, worst, WORST["cs"]))
    # bound: 10x the largest disagreement measured on an MI355X, see DROPIN_MEASURED
    assert worst <= DROPIN_REL, worst


@pytest.mark.parametrize("disc,D,lo,hi", CS_CASES)
@pytest.mark.parametrize("cname,oname,cst,parts", CS_TYPES)
def test_mask(capi, torch, disc, D, lo, hi, cname, oname, cst, parts):
    """Outside |xi| < 0.9 pi / (2 eps_t_sub) the result is bitwise that of the same plan with the setter off; inside it
    is changed; the index set is the drop-in's, point by point."""
    q = cs_signals(D)
    plan = capi.Plan(D, CS_M, q.shape[0], disc)
    try:
        _, off = run(capi, torch, plan, q, cname, Tq=CS_T, XIq=CS_XI)
        assert plan.set_richardson(True) == 0
        rcf, on = run(capi, torch, plan, q, cname, Tq=CS_T, XIq=CS_XI)
        assert rcf == 0
    finally:
        plan.close()
    for b in range(q.shape[0]):
        changed = np.flatnonzero((on[b] != off[b]).any(axis=0))
        assert np.array_equal(changed, np.arange(lo, hi + 1)), changed
        rc1, d1 = capi.fnft_nsev(q[b], CS_T, CS_M, CS_XI, discretization=disc, contspec_type=cname, richardson=True)
        rc0, d0 = capi.fnft_nsev(q[b], CS_T, CS_M, CS_XI, discretization=disc, contspec_type=cname, richardson=False)
        assert rc1 == 0 and rc0 == 0
        d_changed = np.flatnonzero((d1.reshape(parts, CS_M) != d0.reshape(parts, CS_M)).any(axis=0))
        assert np.array_equal(changed, d_changed)


@pytest.mark.parametrize("disc,D", [("2SPLIT4B", 300), ("4SPLIT4A", 256)])
def test_setter_is_a_switch(capi, torch, disc, D):
    """on, off, on: off is the plain plan bit for bit, on is repeatable; the workspace grows at the first enable and
    never after; the plan's last tree run stays the fine one (transfer matrix, evaluation at arbitrary lambda)."""
    q = signals(1, D)
    lam = np.array([0.3 + 0.2j, -1.1 + 0.05j, 0.7j], np.complex128)
    dlam = torch.from_numpy(lam).to("cuda")

    def tree_outputs(plan):
        ev = torch.zeros(3 * plan.eval_len(lam.size, True), dtype=torch.complex128, device="cuda")
        assert plan.eval_device(dlam.data_ptr(), lam.size, ev.data_ptr(), T, derivative=True) == 0
        assert plan.finish() == 0
        tms = [plan.transfer_matrix(b) for b in range(3)]
        assert all(t[0] == 0 for t in tms)
        return ev.cpu().numpy(), [(t[1], t[3]) for t in tms], np.stack([t[2] for t in tms])

    plain = capi.Plan(D, M, 3, disc)
    plan = capi.Plan(D, M, 3, disc)
    try:
        _, ref = run(capi, torch, plain, q, "BOTH")
        ev0, dw0, tm0 = tree_outputs(plain)
        ws0 = plan.workspace_bytes
        assert plan.set_richardson(False) == 0 and plan.workspace_bytes == ws0      # nothing to switch off yet
        _, off0 = run(capi, torch, plan, q, "BOTH")
        assert plan.set_richardson(True) == 0
        ws1 = plan.workspace_bytes
        assert ws1 > ws0
        _, on1 = run(capi, torch, plan, q, "BOTH", calls=2)
        ev1, dw1, tm1 = tree_outputs(plan)
        ws2 = plan.workspace_bytes               # with the evaluation's partials, as on the plain plan
        assert ws2 - ws1 == plain.workspace_bytes - ws0
        assert plan.set_richardson(False) == 0 and plan.workspace_bytes == ws2
        _, off1 = run(capi, torch, plan, q, "BOTH")
        assert plan.set_richardson(True) == 0 and plan.workspace_bytes == ws2
        _, on2 = run(capi, torch, plan, q, "BOTH")
    finally:
        plain.close()
        plan.close()
    assert np.array_equal(off0, ref) and np.array_equal(off1, ref)
    assert np.array_equal(on1, on2) and not np.array_equal(on1, ref)
    assert np.array_equal(ev1, ev0) and dw1 == dw0 and np.array_equal(tm1, tm0)


def test_status_of_the_coarse_pass(capi, torch):
    """2SPLIT2_MODAL, kappa = -1, sech of amplitude 2.5 on 64 samples of [-8, 8]: eps_t |q| reaches 0.635 on the fine grid
    and 1.26 on the coarse one, so only the coarse step fails the check of fnft__akns_fscatter.c:123."""
    disc, D, Ts = "2SPLIT2_MODAL", 64, [-8.0, 8.0]
    q = S.sech_focusing(D, Ts, amp=2.5)[None, :]
    assert capi.fnft_nsev(q[0], Ts, M, XI, kappa=-1, discretization=disc, contspec_type="BOTH", richardson=False)[0] == 0
    assert capi.fnft_nsev(q[0], Ts, M, XI, kappa=-1, discretization=disc, contspec_type="BOTH", richardson=True)[0] != 0
    plan = capi.Plan(D, M, 1, disc)
    try:
        rcf, _ = run(capi, torch, plan, q, "BOTH", kappa=-1, Tq=Ts)
        assert rcf == 0
        assert plan.set_richardson(True) == 0
        rcf, _ = run(capi, torch, plan, q, "BOTH", kappa=-1, Tq=Ts)
        assert rcf == -capi.FNFT_EC_OTHER
        assert plan.set_richardson(False) == 0
        rcf, _ = run(capi, torch, plan, q, "BOTH", kappa=-1, Tq=Ts)
        assert rcf == 0                      # the coarse pass's word was cleared with the plan's
    finally:
        plan.close()


def test_setter_codes(capi, torch):
    kdv = capi.KdvvPlan(64, 16, 1)
    try:
        assert capi.load().fnft_amd_plan_set_richardson(kdv.h, 1) == capi.FNFT_EC_INVALID_ARGUMENT
    finally:
        kdv.close()
    for kw, code in ((dict(D=64, M=0, discretization="2SPLIT4B"), capi.FNFT_EC_INVALID_ARGUMENT),
                     (dict(D=64, M=16, discretization="4SPLIT4A", nskip=2), capi.FNFT_EC_NOT_YET_IMPLEMENTED)):
        plan = capi.Plan(batch=2, **kw)
        try:
            ws = plan.workspace_bytes
            assert plan.set_richardson(True) == code
            assert plan.workspace_bytes == ws
        finally:
            plan.close()
