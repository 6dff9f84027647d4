"""Richardson extrapolation on the batched discrete-spectrum plans (capi.DiscSpecPlan / DiscSpecSearchPlan with
set_richardson: fnft_amd_discspec_plan_set_richardson) on the GPU: every slot against the oracle and against the drop-in
fnft_nsev with richardson_extrapolation_flag = 1 on that signal alone, the accuracy gained over the plain plan, the
output layouts, the guess-free plan, and the independence of the slots with per-signal status."""
import numpy as np
import pytest

import discspec_batch_cases as DC

pytestmark = pytest.mark.gpu
K = 4
# (scheme, D): the fine pass of (2SPLIT4B, 4096) streams its samples while its coarse pass (2048) is staged in LDS
CASES = [("2SPLIT4B", 1024), ("2SPLIT2_MODAL", 1000), ("4SPLIT4A", 512), ("4SPLIT4B", 257), ("2SPLIT4B", 4096)]
ORACLE_BS_ABS, ORACLE_NC_REL = 1e-10, 1e-8          # test_gpu_nsev_batch_discrete.py
# Comparison with the drop-in: both passes of both stop on |err| <= 100 eps and may differ by one last Newton step, and
# the step (sn x - x_s) / (sn - 1) amplifies a difference of the two passes by up to (sn + 1) / (sn - 1).  Largest
# disagreement measured on an MI355X over every comparison with the drop-in in this file (each prints its figures):
# bound states 1.780e-15 absolute, norming constants and residues 6.955e-14 relative.  The bounds are 10x that, never
# above the oracle's.
DROPIN_BS_MEASURED, DROPIN_NC_MEASURED = 1.780e-15, 6.955e-14
DROPIN_BS_ABS, DROPIN_NC_REL = min(10 * DROPIN_BS_MEASURED, ORACLE_BS_ABS), min(10 * DROPIN_NC_MEASURED, ORACLE_NC_REL)
GAIN = 10.0      # the oracle alone gains at least 14x (4SPLIT4B, D = 257) and more than 100x from D = 1024


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


def opts_of(disc, **kw):
    o = {"discretization": disc, "bound_state_localization": "NEWTON", "bound_state_filtering": "FULL", "niter": 10,
         "discspec_type": "BOTH"}
    o.update(kw)
    return o


def run_plan(capi, torch, q, g, opts, richardson=True, want_nc=True, Kc=K, calls=1):
    """One plan (a guess plan, or with g None a guess-free one): (rc of finish, bs[B, K], nc[B, W] or None, K_out[B],
    status[B]) of `calls` identical calls.  The workspace grows at the first enable and on no call."""
    q = np.ascontiguousarray(q, np.complex128)
    B, D = q.shape
    plan = capi.DiscSpecPlan(D, Kc, B, opts) if g is not None else capi.DiscSpecSearchPlan(D, Kc, B, opts)
    try:
        W = plan.nc_len()
        ws0 = plan.workspace_bytes()
        if richardson:
            assert plan.set_richardson(True) == 0
            assert plan.workspace_bytes() > ws0
            assert plan.set_richardson(False) == 0 and plan.set_richardson(True) == 0
        ws = plan.workspace_bytes()
        dq = torch.from_numpy(q.reshape(-1)).to("cuda")
        dg = None if g is None else torch.from_numpy(np.ascontiguousarray(g, np.complex128).reshape(-1)).to("cuda")
        res = []
        for _ in range(calls):
            dbs = torch.zeros(B * Kc, dtype=torch.complex128, device="cuda")
            dnc = torch.zeros(B * W, dtype=torch.complex128, device="cuda") if want_nc else None
            dk = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            args = (dbs.data_ptr(), dnc.data_ptr() if want_nc else 0, dk.data_ptr())
            rc = plan.run_device(dq.data_ptr(), list(DC.T), *((dg.data_ptr(),) if g is not None else ()), *args)
            assert rc == 0, (rc, capi.last_error())
            rcf, st, ko = plan.finish()
            assert plan.workspace_bytes() == ws
            kd = dk.cpu().numpy()
            assert np.array_equal(kd.astype(np.uint64), ko)
            res.append((dbs.cpu().numpy().reshape(B, Kc), dnc.cpu().numpy().reshape(B, W) if want_nc else None, kd))
        assert np.array_equal(dq.cpu().numpy().reshape(B, D), q, equal_nan=True)
        for a in res[1:]:
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, res[0]) if x is not None)
        bs, nc, kd = res[0]
        for b in range(B):
            if st[b] == 0:
                k = int(kd[b])
                assert 0 <= k <= Kc and not np.isnan(bs[b, :k]).any() and np.isnan(bs[b, k:]).all()
                if nc is not None:
                    for part in range(W // Kc):
                        assert not np.isnan(nc[b, part * Kc:part * Kc + k]).any()
                        assert np.isnan(nc[b, part * Kc + k:(part + 1) * Kc]).all()
    finally:
        plan.close()
    return rcf, bs, nc, kd, st


_RUNS = {}


def batched(capi, torch, disc, D, richardson=True):
    """The result of one of CASES (FULL, niter = 10, BOTH), computed once."""
    key = (disc, D, richardson)
    if key not in _RUNS:
        q, g = DC.batch(D, K, disc.startswith("4SPLIT"))
        _RUNS[key] = run_plan(capi, torch, q, g, opts_of(disc), richardson, calls=2 if richardson else 1)
    return _RUNS[key]


def errors(bs, nc, k, ref_bs, ref_nc, ref_res, Kc=K):
    assert k == ref_bs.size, (k, bs, ref_bs)
    e_bs = np.abs(bs[:k] - ref_bs).max()
    e_nc = max((np.abs(nc[:k] - ref_nc) / np.abs(ref_nc)).max(), (np.abs(nc[Kc:Kc + k] - ref_res) / np.abs(ref_res)).max())
    return e_bs, e_nc


@pytest.mark.parametrize("disc,D", CASES)
def test_against_the_oracle(capi, torch, oracle, disc, D):
    rcf, bs, nc, ko, st = batched(capi, torch, disc, D)
    assert rcf == 0 and not st.any()
    assert list(ko) == DC.K_OUT
    q, g = DC.batch(D, K, disc.startswith("4SPLIT"))
    worst = [0.0, 0.0]
    for b in range(len(DC.PAIRS)):
        rc, bs_o, nc_o, res_o = oracle.fnft_nsev_ds(q[b], DC.T, disc, bsloc="NEWTON", bsfilt="FULL", niter=10,
                                                    guesses=g[b], richardson=True)
        assert rc == 0
        e = errors(bs[b], nc[b], int(ko[b]), bs_o, nc_o, res_o)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        assert e[0] < ORACLE_BS_ABS and e[1] < ORACLE_NC_REL, (b, e)
    print("vs oracle %s D=%d: bound states %.3e abs, norming constants / residues %.3e rel" % (disc, D, *worst))


WORST = {"bs": 0.0, "nc": 0.0}


@pytest.mark.parametrize("disc,D", CASES)
def test_against_the_drop_in(capi, torch, disc, D):
    rcf, bs, nc, ko, st = batched(capi, torch, disc, D)
    q, g = DC.batch(D, K, disc.startswith("4SPLIT"))
    worst = [0.0, 0.0]
    for b in range(len(DC.PAIRS)):
        rc, bs_d, nc_d, res_d = capi.fnft_nsev_ds(q[b], DC.T, discretization=disc, bsloc="NEWTON", guesses=g[b],
                                                  richardson=True)
        assert rc == 0 == st[b]
        e = errors(bs[b], nc[b], int(ko[b]), bs_d, nc_d, res_d)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    WORST["bs"], WORST["nc"] = max(WORST["bs"], worst[0]), max(WORST["nc"], worst[1])
    print("vs drop-in %s D=%d: bound states %.3e abs, norming constants / residues %.3e rel; worst so far %.3e, %.3e"
          % (disc, D, *worst, WORST["bs"], WORST["nc"]))
    # bounds: 10x the largest disagreement measured on an MI355X, see DROPIN_*
    assert worst[0] < DROPIN_BS_ABS and worst[1] < DROPIN_NC_REL, worst


@pytest.mark.parametrize("disc,D", CASES)
def test_accuracy_gain(capi, torch, disc, D):
    """Every signal's largest eigenvalue error against the closed form falls by at least 10x."""
    _, bs1, _, ko1, _ = batched(capi, torch, disc, D)
    _, bs0, _, ko0, _ = batched(capi, torch, disc, D, richardson=False)
    assert np.array_equal(ko1, ko0)
    for b, (A, c) in enumerate(DC.PAIRS):
        ex = DC.exact_eigenvalues(A, c)
        k = int(ko1[b])
        assert k == ex.size
        e1 = max(np.abs(bs1[b, :k] - x).min() for x in ex)
        e0 = max(np.abs(bs0[b, :k] - x).min() for x in ex)
        print("%s D=%d signal %d: error %.3e plain, %.3e extrapolated, gain %.1f" % (disc, D, b, e0, e1, e0 / e1))
        assert e1 * GAIN <= e0, (b, e0, e1)


def test_output_layouts(capi, torch):
    disc, D = "2SPLIT4B", 1024
    q, g = DC.batch(D, K, False)
    _, bs, both, ko, _ = batched(capi, torch, disc, D)
    _, bs_off, both_off, _, _ = batched(capi, torch, disc, D, richardson=False)
    rcf, bs0, nc0, ko0, _ = run_plan(capi, torch, q, g, opts_of(disc, discspec_type="NORMING_CONSTANTS"))
    assert rcf == 0 and nc0.shape == (len(DC.PAIRS), K)
    assert np.array_equal(nc0, both_off[:, :K], equal_nan=True)      # norming constants: those of the plain plan
    assert np.array_equal(nc0, both[:, :K], equal_nan=True)
    rcf, bs1, nc1, ko1, _ = run_plan(capi, torch, q, g, opts_of(disc, discspec_type="RESIDUES"))
    assert rcf == 0 and np.array_equal(nc1, both[:, K:], equal_nan=True)
    rcf, bsn, ncn, kon, _ = run_plan(capi, torch, q, g, opts_of(disc), want_nc=False)
    assert rcf == 0 and ncn is None
    for x, k in ((bs0, ko0), (bs1, ko1), (bsn, kon)):
        assert np.array_equal(x, bs, equal_nan=True) and np.array_equal(k, ko)
    for b in range(len(DC.PAIRS)):
        k = int(ko[b])
        assert (bs[b, :k] != bs_off[b, :k]).all() and (both[b, K:K + k] != both_off[b, K:K + k]).all()


def test_search_plan(capi, torch, oracle):
    """The guess-free plan with the default options (SUBSAMPLE_AND_REFINE), as sets per signal."""
    D, Kc = 1024, 6
    q = np.stack([DC.signal(D, A, c) for A, c in DC.PAIRS])
    o = {"discspec_type": "BOTH"}
    rcf, bs, nc, ko, st = run_plan(capi, torch, q, None, o, Kc=Kc)
    rcf0, bs0, nc0, ko0, st0 = run_plan(capi, torch, q, None, o, richardson=False, Kc=Kc)
    assert rcf == 0 and rcf0 == 0 and not st.any() and np.array_equal(ko, ko0)
    worst = [0.0, 0.0]
    for b in range(len(DC.PAIRS)):
        rc, bs_o, nc_o, res_o = oracle.fnft_nsev_ds(q[b], DC.T, richardson=True)
        assert rc == 0
        k = int(ko[b])
        assert k == bs_o.size == DC.K_OUT[b]
        order = [int(np.abs(bs[b, :k] - x).argmin()) for x in bs_o]
        assert sorted(order) == list(range(k))
        e = errors(bs[b, order], np.concatenate([nc[b, :Kc][order], np.zeros(Kc - k), nc[b, Kc:][order]]), k, bs_o, nc_o,
                   res_o, Kc)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        assert e[0] < ORACLE_BS_ABS and e[1] < ORACLE_NC_REL, (b, e)
        assert (bs[b, :k] != bs0[b, :k]).all()
    print("search plan vs oracle: bound states %.3e abs, norming constants / residues %.3e rel" % tuple(worst))


def test_failing_slot(capi, torch):
    """One signal with a NaN sample: its status is non-zero, every other slot is bitwise what it is without it."""
    disc, D = "2SPLIT4B", 1024
    q, g = DC.batch(D, K, False)
    _, bs, nc, ko, _ = batched(capi, torch, disc, D)
    bad = 5
    q2 = q.copy()
    q2[bad, 300] = np.nan
    rcf, bs2, nc2, ko2, st2 = run_plan(capi, torch, q2, g, opts_of(disc))
    assert rcf != 0 and st2[bad] != 0
    ok = [b for b in range(len(DC.PAIRS)) if b != bad]
    assert not st2[ok].any()
    assert np.array_equal(bs2[ok], bs[ok], equal_nan=True) and np.array_equal(nc2[ok], nc[ok], equal_nan=True)
    assert np.array_equal(ko2[ok], ko[ok])
