"""Every level path of the product tree on the GPU against the extended-precision reference (tests/tree_ref.py).

Each case of tests/tree_cases.py runs through its entry point; the result is evaluated at K points of the unit circle
and compared with the exact ordered product of the factors there.  Plan cases also check the launched kernels against
the case's list (the emulator's schedule test checks the same list without a GPU)."""
import json
import os

import numpy as np
import pytest

import tree_cases as TC
import tree_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_measured = {}


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    yield c
    out = os.environ.get("FNFT_TREE_ERR_JSON")   # optional record of the measured errors
    if out:
        with open(out, "w") as f:
            json.dump(_measured, f, indent=1)


def _check(c, key, res, W, ref, m, n_factors, C):
    e = R.error(res, W, ref, m)
    N = int(2 ** np.ceil(np.log2(res.shape[1])))   # longest transform of the tree: the top level's product length
    b = R.err_bound(C, N, n_factors)
    _measured[key] = dict(e=e, bound=b, e_over_u_log2N=e / R.err_bound((1.0, 0.0), N), e_over_u_n=e / (R.U * n_factors))
    assert e < b, (key, e, b)


@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_ids())
def test_tree_path(capi, oracle, case):
    import torch
    c = case
    m = R.points(c["K"] or (16 if c["n"] * (c["disc"] if c["entry"] == "fmult" else 4) <= (1 << 16) else 6))
    if c["entry"] == "fmult":
        p = TC.fmult_factors(c)
        rc, d, res, W = capi.poly_fmult2x2(c["disc"], c["n"], p)
        assert rc == 0, capi.last_error()
        assert d == c["disc"] * c["n"]
        if c["shift"]:
            assert W != 0
        _check(c, c["id"], res, W, R.tree_ref(p * 2.0 ** -c["shift"], c["disc"], c["n"], m, c["shift"]), m, c["n"],
               TC.BOUND_GENERAL)
    elif c["entry"] == "akns":
        q, r, T = TC.akns_signal(c)
        eps_t = (T[1] - T[0]) / (q.size - 1)
        rc, d, res, W = capi.akns_fscatter(q, r, eps_t, c["disc"])
        assert rc == 0, capi.last_error()
        rc2, deg0, f = oracle.akns_coeffs(q, r, eps_t, c["disc"])
        assert rc2 == 0 and d == deg0 * q.size
        _check(c, c["id"], res, W, R.tree_ref(f, deg0, q.size, m), m, q.size, TC.BOUND_SAMPLES)
    elif c["entry"] == "kdv":
        u, T = TC.kdv_signal(c)
        eps_t = (T[1] - T[0]) / (u.size - 1)
        rc, d, res, W = capi.kdv_fscatter(u, eps_t, c["disc"])
        assert rc == 0, capi.last_error()
        rc2, deg0, f = oracle.akns_coeffs(u, -np.ones_like(u), eps_t, c["disc"])
        assert rc2 == 0 and d == deg0 * u.size
        _check(c, c["id"], res, W, R.tree_ref(f, deg0, u.size, m), m, u.size, TC.BOUND_REAL)
    else:
        B, D, M = c["batch"], c["n"], 64
        sig = [TC.plan_signal(c, k) for k in range(B)]
        T = sig[0][1]
        plan = capi.Plan(D, M, batch=B, discretization=c["disc"])
        dq = torch.from_numpy(np.concatenate([s[0] for s in sig])).cuda()
        out = torch.zeros(B * 3 * M, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        plan.set_launch_timing(True)
        rc = plan.contspec_device(dq.data_ptr(), out.data_ptr(), T, [-2.0, 2.0], kappa=1, contspec_type="BOTH")
        assert rc == 0, capi.last_error()
        assert plan.finish() == 0
        names = [n.replace(" ", "") for n, _ in plan.launch_times()]
        missing = [k for k in c["kernels"] if k not in names]
        assert not missing, (missing, names)
        eps_t = (T[1] - T[0]) / (D - 1)
        for b in range(B):
            rc, d, res, W = plan.transfer_matrix(b)
            assert rc == 0, capi.last_error()
            q = sig[b][0]
            rc2, deg0, f = oracle.akns_coeffs(q, -np.conj(q), eps_t, c["disc"])
            assert rc2 == 0 and d == deg0 * D
            _check(c, "%s[b=%d]" % (c["id"], b), res, W, R.tree_ref(f, deg0, D, m), m, D, TC.BOUND_SAMPLES)
            del res, f
        plan.close()

