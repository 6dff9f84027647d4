"""The batched discrete spectrum of fnft_nsev (capi.DiscSpecPlan: fnft_amd_discspec_plan_* /
fnft_amd_nsev_discspec_device) on the GPU: every slot against the oracle and against the drop-in fnft_nsev run on that
signal alone, the options and output layouts, independence of the slots with per-signal status, both sample sources
(LDS-resident up to 2048 preprocessed samples, streaming above), a batch beyond 65535 workgroups, streams."""

import numpy as np
import pytest

import discspec_batch_cases as DC

pytestmark = pytest.mark.gpu
FNFT_EC_INVALID_ARGUMENT = 2
K = 4
# (scheme, D): D <= 2048 (1024 for 4SPLIT4A/B, two samples per grid point) is staged in LDS, 4096 streams
CASES = [("2SPLIT4B", 1024), ("2SPLIT2A", 2048), ("2SPLIT2_MODAL", 1000), ("4SPLIT4A", 512), ("4SPLIT4B", 512),
         ("4SPLIT4A", 1024), ("4SPLIT4B", 1024), ("2SPLIT4B", 4096), ("4SPLIT4B", 2048)]
# Bounds of the comparison with the oracle: the project's bounds for this comparison (test_gpu_parity.py)
ORACLE_BS_ABS, ORACLE_NC_REL = 1e-10, 1e-8
# Bounds of the comparison with the drop-in: both stop on |err| <= 100 eps and may differ by one last Newton step, and
# the maps are combined in another order.  Largest disagreement measured on an MI355X over every comparison with the
# drop-in in this file (each prints its figures): bound states 9.305e-16 absolute, norming constants and residues
# 6.840e-14 relative.  The bounds are 10x that, far below the oracle bounds.
DROPIN_BS_MEASURED, DROPIN_NC_MEASURED = 9.305e-16, 6.840e-14
DROPIN_BS_ABS, DROPIN_NC_REL = 10 * DROPIN_BS_MEASURED, 10 * DROPIN_NC_MEASURED
assert DROPIN_BS_ABS <= ORACLE_BS_ABS and DROPIN_NC_REL <= ORACLE_NC_REL


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


def run_plan(capi, torch, q, g, opts, want_nc=True, stream=None, calls=1):
    """One plan, `calls` calls: (rc of finish, bs[B, K], nc[B, W] or None, K_out[B], status[B]).  Checks that the inputs
    are unchanged, that finish reports the device's counts, that the tails are NaN and that the workspace does not move."""
    q, g = np.ascontiguousarray(q, np.complex128), np.ascontiguousarray(g, np.complex128)
    B, D = q.shape
    Kc = g.shape[1]
    plan = capi.DiscSpecPlan(D, Kc, B, opts)
    try:
        W = plan.nc_len()
        ws = plan.workspace_bytes()
        assert ws > 0
        dq = torch.from_numpy(q.reshape(-1)).to("cuda")
        dg = torch.from_numpy(g.reshape(-1)).to("cuda")
        sp = 0 if stream is None else stream.cuda_stream
        outs = []
        for _ in range(calls):
            dbs = torch.zeros(B * Kc, dtype=torch.complex128, device="cuda")
            dnc = torch.zeros(B * W, dtype=torch.complex128, device="cuda") if want_nc else None
            dk = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = plan.run_device(dq.data_ptr(), list(DC.T), dg.data_ptr(), dbs.data_ptr(),
                                 dnc.data_ptr() if want_nc else 0, dk.data_ptr(), sp)
            assert rc == 0, (rc, capi.last_error())
            outs.append((dbs, dnc, dk))
        rcf, st, ko = plan.finish(sp)
        assert plan.workspace_bytes() == ws
        assert np.array_equal(dq.cpu().numpy().reshape(B, D), q) and np.array_equal(dg.cpu().numpy().reshape(B, Kc), g)
        res = []
        for dbs, dnc, dk in outs:
            bs = dbs.cpu().numpy().reshape(B, Kc)
            nc = dnc.cpu().numpy().reshape(B, W) if want_nc else None
            kd = dk.cpu().numpy()
            assert np.array_equal(kd.astype(np.uint64), ko)
            res.append((bs, nc, kd))
        for a in res[1:]:     # calls on one plan back to back: identical results
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, res[0]) if x is not None)
        bs, nc, kd = res[0]
        for b in range(B):
            if st[b] != 0:
                continue
            k = int(kd[b])
            assert 0 <= k <= Kc and not np.isnan(bs[b, :k]).any() and np.isnan(bs[b, k:]).all()
            if nc is not None:
                for part in range(W // Kc):
                    assert np.isnan(nc[b, part * Kc + k:(part + 1) * Kc]).all()
    finally:
        plan.close()
    return rcf, bs, nc, kd, st


_RUNS = {}


def batched(capi, torch, disc, D):
    """The batched result of one of CASES (FULL, niter = 10, BOTH), computed once."""
    if (disc, D) not in _RUNS:
        q, g = DC.batch(D, K, disc.startswith("4SPLIT"))
        _RUNS[(disc, D)] = run_plan(capi, torch, q, g, opts_of(disc))
    return _RUNS[(disc, D)]


def drop_in(capi, disc, q, g, **kw):
    """fnft_nsev on one signal: (rc, bs, nc, res)."""
    return capi.fnft_nsev_ds(q, DC.T, discretization=disc, bsloc="NEWTON", guesses=g, **kw)


WORST = {"bs": 0.0, "nc": 0.0}     # largest disagreement with the drop-in seen by this run (printed by every test)


def compare(bs, nc, k, ref_bs, ref_nc, ref_res, bs_abs, nc_rel, Kc, drop=True):
    """Largest disagreements (bound states absolute; norming constants and residues relative), asserted against the
    bounds.  nc: the BOTH layout, residues at the capacity Kc."""
    assert k == ref_bs.size, (k, bs, ref_bs)
    if k == 0:
        return 0.0, 0.0
    e_bs = np.abs(bs[:k] - ref_bs).max()
    e_nc = (np.abs(nc[:k] - ref_nc) / np.abs(ref_nc)).max()
    e_res = (np.abs(nc[Kc:Kc + k] - ref_res) / np.abs(ref_res)).max()
    if drop:
        WORST["bs"], WORST["nc"] = max(WORST["bs"], e_bs), max(WORST["nc"], e_nc, e_res)
        print("vs drop-in: bound states %.3e abs, norming constants / residues %.3e rel; worst so far %.3e, %.3e"
              % (e_bs, max(e_nc, e_res), WORST["bs"], WORST["nc"]))
    assert e_bs < bs_abs and e_nc < nc_rel and e_res < nc_rel, (e_bs, e_nc, e_res, bs[:k], ref_bs)
    return e_bs, max(e_nc, e_res)


@pytest.mark.parametrize("disc,D", CASES)
def test_against_the_oracle(capi, torch, oracle, disc, D):
    rcf, bs, nc, ko, st = batched(capi, torch, disc, D)
    assert rcf == 0 and not st.any()
    assert list(ko) == DC.K_OUT
    worst = [0.0, 0.0]
    for b, (rc, bs_o, nc_o, res_o, a_o) in enumerate(DC.oracle_reference(oracle, disc, D, K)):
        assert rc == 0
        # b = phi/psi is independent of the grid point only at a zero of a: with these inputs every one converges
        assert (a_o < 1e-9).all(), (b, a_o)
        e = compare(bs[b], nc[b], int(ko[b]), bs_o, nc_o, res_o, ORACLE_BS_ABS, ORACLE_NC_REL, K, drop=False)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("vs oracle %s D=%d: bound states %.3e abs, norming constants / residues %.3e rel" % (disc, D, *worst))


@pytest.mark.parametrize("disc,D", CASES)
def test_against_the_drop_in(capi, torch, disc, D):
    rcf, bs, nc, ko, st = batched(capi, torch, disc, D)
    q, g = DC.batch(D, K, disc.startswith("4SPLIT"))
    worst = [0.0, 0.0]
    for b in range(len(DC.PAIRS)):
        rc, bs_d, nc_d, res_d = drop_in(capi, disc, q[b], g[b])
        assert rc == 0 == st[b]
        # bounds: 10x the largest disagreement measured on an MI355X (9.305e-16 abs, 6.840e-14 rel), see DROPIN_*
        e = compare(bs[b], nc[b], int(ko[b]), bs_d, nc_d, res_d, DROPIN_BS_ABS, DROPIN_NC_REL, K)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("vs drop-in %s D=%d: bound states %.3e abs, norming constants / residues %.3e rel" % (disc, D, *worst))


def test_discspec_types(capi, torch):
    """NORMING_CONSTANTS and RESIDUES alone are the two halves of BOTH; no output array at all changes nothing else."""
    disc, D = "2SPLIT4B", 1024
    q, g = DC.batch(D, K, False)
    _, bs, both, ko, _ = batched(capi, torch, disc, D)
    for dstype, part in (("NORMING_CONSTANTS", both[:, :K]), ("RESIDUES", both[:, K:])):
        rcf, bs1, nc1, ko1, st1 = run_plan(capi, torch, q, g, opts_of(disc, discspec_type=dstype))
        assert rcf == 0 and nc1.shape == (len(DC.PAIRS), K)
        assert np.array_equal(bs1, bs, equal_nan=True) and np.array_equal(ko1, ko)
        assert np.array_equal(nc1, part, equal_nan=True)
    rcf, bs0, nc0, ko0, st0 = run_plan(capi, torch, q, g, opts_of(disc), want_nc=False)
    assert rcf == 0 and nc0 is None and np.array_equal(bs0, bs, equal_nan=True) and np.array_equal(ko0, ko)


@pytest.mark.parametrize("bsfilt", ["NONE", "BASIC"])
def test_filters(capi, torch, bsfilt):
    disc, D = "2SPLIT4B", 1024
    q, g = DC.batch(D, K, False)
    rcf, bs, nc, ko, st = run_plan(capi, torch, q, g, opts_of(disc, bound_state_filtering=bsfilt))
    assert rcf == 0 and not st.any()
    for b, (A, c) in enumerate(DC.PAIRS):
        rc, bs_d, nc_d, res_d = drop_in(capi, disc, q[b], g[b], bsfilt=bsfilt)
        assert rc == 0
        if bsfilt == "NONE":
            # nothing is filtered or merged: all K slots come back in order.  The start values below the real axis
            # have no eigenvalue to converge to and are not compared
            n = min(K, DC.K_OUT[b] + 1)
            assert ko[b] == K == bs_d.size
            head = np.concatenate([nc[b, :n], np.zeros(K - n), nc[b, K:K + n]])
            compare(bs[b, :n], head, n, bs_d[:n], nc_d[:n], res_d[:n], DROPIN_BS_ABS, DROPIN_NC_REL, K)
        else:
            assert ko[b] == DC.K_OUT[b]
            compare(bs[b], nc[b], int(ko[b]), bs_d, nc_d, res_d, DROPIN_BS_ABS, DROPIN_NC_REL, K)


@pytest.mark.parametrize("skewed", [False, True])
def test_no_iterations(capi, torch, skewed):
    """niter = 0: norming constants and residues at the caller's eigenvalues (fnft__nse_scatter_bound_states there).
    Away from a zero of a, b = phi1/psi1 depends on the grid point the metric picks.  |q| of the chirped sech pulses is
    even in t and the grid is symmetric, so the metric has the same value at mirrored grid points and rounding picks the
    side (the drop-in and the oracle differ there too): on those pulses only a' = b / residue, which is the same on both
    sides, is compared.  With the envelope skewed by 1 + 0.3 tanh(t) the minimum is unique and b and the residues are
    compared themselves."""
    disc, D = "2SPLIT4B", 1024
    q, g = DC.batch(D, K, False)
    if skewed:
        q = q * (1.0 + 0.3 * np.tanh(DC.S.tgrid(DC.T, D)))[None, :]
    rcf, bs, nc, ko, st = run_plan(capi, torch, q, g, opts_of(disc, niter=0, bound_state_filtering="NONE"))
    assert rcf == 0 and not st.any() and (ko == K).all()
    assert np.array_equal(bs, g)
    for b in range(len(DC.PAIRS)):
        rc, a, ap, bb = capi.nse_scatter_bound_states(q[b], DC.T, g[b])
        assert rc == 0
        e = (np.abs(nc[b, :K] / nc[b, K:] - ap) / np.abs(ap)).max()
        if skewed:
            e = max(e, (np.abs(nc[b, :K] - bb) / np.abs(bb)).max(), (np.abs(nc[b, K:] - bb / ap) / np.abs(bb / ap)).max())
        WORST["nc"] = max(WORST["nc"], e)
        print("niter = 0, skewed %d, signal %d: %.3e rel; worst so far %.3e" % (skewed, b, e, WORST["nc"]))
        assert e < DROPIN_NC_REL, (b, nc[b], bb, ap)


def test_slots_are_independent(capi, torch):
    """Permuting the slots permutes the results exactly."""
    disc, D = "2SPLIT4B", 1024
    q, g = DC.batch(D, K, False)
    _, bs, nc, ko, _ = batched(capi, torch, disc, D)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    rcf, bs_p, nc_p, ko_p, st_p = run_plan(capi, torch, q[perm], g[perm], opts_of(disc))
    assert rcf == 0
    assert np.array_equal(bs_p, bs[perm], equal_nan=True) and np.array_equal(nc_p, nc[perm], equal_nan=True)
    assert np.array_equal(ko_p, ko[perm])


def test_failing_slot(capi, torch):
    """A signal that violates the step-size check of 2SPLIT2_MODAL: its slot reports what fnft_nsev returns for it, the
    other slots are what they are without it."""
    disc, D = "2SPLIT2_MODAL", 1000
    q, g = DC.batch(D, K, False)
    _, bs, nc, ko, _ = batched(capi, torch, disc, D)
    bad = 3
    q2 = q.copy()
    q2[bad] = DC.signal(D, 25.0, 0.0)        # purely imaginary samples with eps_t |q| >= 1 around t = 0
    rc_d = drop_in(capi, disc, q2[bad], g[bad])[0]
    assert rc_d != 0
    rcf, bs2, nc2, ko2, st2 = run_plan(capi, torch, q2, g, opts_of(disc))
    assert rcf == rc_d and st2[bad] == rc_d
    ok = [b for b in range(len(DC.PAIRS)) if b != bad]
    assert not st2[ok].any()
    assert np.array_equal(bs2[ok], bs[ok], equal_nan=True) and np.array_equal(nc2[ok], nc[ok], equal_nan=True)
    assert np.array_equal(ko2[ok], ko[ok])


def test_more_workgroups_than_a_16_bit_grid(capi, torch):
    """batch*K = 80000 (signal, eigenvalue) pairs: every slot equals the slot of the 8-signal batch it repeats."""
    disc, D, reps = "2SPLIT4B", 64, 2500
    q, g = DC.batch(D, K, False)
    rc8, bs8, nc8, ko8, st8 = run_plan(capi, torch, q, g, opts_of(disc))
    rcf, bs, nc, ko, st = run_plan(capi, torch, np.tile(q, (reps, 1)), np.tile(g, (reps, 1)), opts_of(disc))
    assert rcf == rc8 == 0 and not st.any()
    assert np.array_equal(bs, np.tile(bs8, (reps, 1)), equal_nan=True)
    assert np.array_equal(nc, np.tile(nc8, (reps, 1)), equal_nan=True)
    assert np.array_equal(ko, np.tile(ko8, reps))


@pytest.mark.parametrize("D,Kc", [(2049, 4), (1024, 1), (2048, 1)])
def test_sizes(capi, torch, D, Kc):
    """The first size that streams (odd, not a power of two), and a single eigenvalue slot."""
    disc = "2SPLIT4B"
    q, g = DC.batch(D, Kc, False)
    rcf, bs, nc, ko, st = run_plan(capi, torch, q, g, opts_of(disc))
    assert rcf == 0 and not st.any()
    for b in range(len(DC.PAIRS)):
        rc, bs_d, nc_d, res_d = drop_in(capi, disc, q[b], g[b])
        assert rc == 0
        compare(bs[b], nc[b], int(ko[b]), bs_d, nc_d, res_d, DROPIN_BS_ABS, DROPIN_NC_REL, Kc)


def test_streams_and_repeated_calls(capi, torch):
    disc, D = "4SPLIT4B", 512
    q, g = DC.batch(D, K, True)
    _, bs, nc, ko, _ = batched(capi, torch, disc, D)
    s = torch.cuda.Stream()
    rcf, bs_s, nc_s, ko_s, st_s = run_plan(capi, torch, q, g, opts_of(disc), stream=s, calls=2)
    assert rcf == 0
    assert np.array_equal(bs_s, bs, equal_nan=True) and np.array_equal(nc_s, nc, equal_nan=True)
    assert np.array_equal(ko_s, ko)


def test_call_codes(capi, torch):
    """NULL arrays and a bad T are refused before anything is enqueued."""
    plan = capi.DiscSpecPlan(64, 2, 2, opts_of("2SPLIT4B"))
    try:
        buf = torch.zeros(2 * 64, dtype=torch.complex128, device="cuda")
        p = buf.data_ptr()
        T = list(DC.T)
        assert plan.run_device(0, T, p, p, p, p) == FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(p, T, 0, p, p, p) == FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(p, T, p, 0, p, p) == FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(p, T, p, p, p, 0) == FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(p, None, p, p, p, p) == FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(p, [1.0, 1.0], p, p, p, p) == FNFT_EC_INVALID_ARGUMENT
        assert plan.run_device(p, [2.0, 1.0], p, p, p, p) == FNFT_EC_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert (buf == 0).all()
    finally:
        plan.close()
