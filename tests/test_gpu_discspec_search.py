"""The guess-free batched discrete spectrum of fnft_nsev (capi.DiscSpecSearchPlan: fnft_amd_discspec_search_plan_* /
fnft_amd_nsev_discspec_search_device) on the GPU: every slot against the oracle and against the drop-in fnft_nsev run on
that signal alone, the options and output layouts, independence of the slots with per-signal status, truncation to K,
a batch of 20000 signals on the folded grid axis, streams, call codes.

A signal's bound states come in the root finder's order, so every comparison matches values by nearest neighbour."""

import ctypes

import numpy as np
import pytest

import discspec_batch_cases as DC

pytestmark = pytest.mark.gpu
FNFT_EC_INVALID_ARGUMENT = 2
K = 8
SAR, FE = "SUBSAMPLE_AND_REFINE", "FAST_EIGENVALUE"
# Bounds of the comparison with the oracle: the project's bounds for this comparison (test_emu_kernels.py,
# test_gpu_parity.py): after a Newton refinement, and for the unrefined roots of a degree-D polynomial
ORACLE_BS_ABS, ORACLE_NC_REL, ORACLE_FE_ABS = 1e-10, 1e-8, 1e-6
# Bounds of the comparison with the drop-in: both sides run Newton to the same stop (|err| <= 100 eps) from start values
# that differ in the last digits (the root finder's sums are segmented differently), and may differ by one last step.
# Largest disagreement measured on an MI355X over every comparison with the drop-in in this file (each prints its
# figures): bound states 9.156e-16 absolute (2SPLIT4B, D = 1024), norming constants and residues 1.416e-13 relative
# (2SPLIT4B, D = 4096).  The bounds are 10x that and must stay at or below the oracle bounds.
DROPIN_BS_MEASURED, DROPIN_NC_MEASURED = 9.156e-16, 1.416e-13
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


def opts_of(disc, bsloc=SAR, **kw):
    o = {"discretization": disc, "bound_state_localization": bsloc, "bound_state_filtering": "FULL", "niter": 10,
         "discspec_type": "BOTH"}
    o.update(kw)
    return o


def signals(D, pairs=DC.PAIRS):
    return np.stack([DC.signal(D, A, c) for A, c in pairs])


def run_plan(capi, torch, q, Kc, opts, want_nc=True, stream=None, calls=1, finite=True):
    """One plan, `calls` calls: (rc of finish, bs[B, K], nc[B, W] or None, K_out[B], status[B], warnings[B]).  Checks that
    the input is unchanged, that finish reports the device's counts, that the tails are NaN, that calls on one plan give
    bitwise equal results and that the workspace does not move.  finite = False: without a filter the values may be anything
    (roots at infinity map to NaN)."""
    q = np.ascontiguousarray(q, np.complex128)
    B, D = q.shape
    plan = capi.DiscSpecSearchPlan(D, Kc, B, opts)
    try:
        W = plan.nc_len()
        ws = plan.workspace_bytes()
        assert ws > 0 and plan.roots()[0] > 0
        dq = torch.from_numpy(q.reshape(-1)).to("cuda")
        sp = 0 if stream is None else stream.cuda_stream
        outs = []
        for _ in range(calls):
            dbs = torch.zeros(B * Kc, dtype=torch.complex128, device="cuda")
            dnc = torch.zeros(B * W, dtype=torch.complex128, device="cuda") if want_nc else None
            dk = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = plan.run_device(dq.data_ptr(), list(DC.T), dbs.data_ptr(), dnc.data_ptr() if want_nc else 0,
                                 dk.data_ptr(), sp)
            assert rc == 0, (rc, capi.last_error())
            outs.append((dbs, dnc, dk))
        rcf, st, ko = plan.finish(sp)
        wn = plan.warnings()
        assert plan.workspace_bytes() == ws
        assert np.array_equal(dq.cpu().numpy().reshape(B, D), q)
        res = []
        for dbs, dnc, dk in outs:
            bs = dbs.cpu().numpy().reshape(B, Kc)
            nc = dnc.cpu().numpy().reshape(B, W) if want_nc else None
            kd = dk.cpu().numpy()
            assert np.array_equal(kd.astype(np.uint64), ko)
            res.append((bs, nc, kd))
        for a in res[1:]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, res[0]) if x is not None)
        bs, nc, kd = res[0]
        for b in range(B):
            if st[b] != 0:
                continue
            k = int(kd[b])
            assert 0 <= k <= Kc and (not finite or not np.isnan(bs[b, :k]).any()) and np.isnan(bs[b, k:]).all()
            if nc is not None:
                for part in range(W // Kc):
                    assert np.isnan(nc[b, part * Kc + k:(part + 1) * Kc]).all()
    finally:
        plan.close()
    return rcf, bs, nc, kd, st, wn


_RUNS = {}


def batched(capi, torch, disc, D, bsloc=SAR, Kc=K, **kw):
    """The result on the eight pulses (FULL, niter = 10, BOTH unless kw says otherwise), computed once and never modified."""
    key = (disc, D, bsloc, Kc, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = run_plan(capi, torch, signals(D), Kc, opts_of(disc, bsloc, **kw))
    return _RUNS[key]


def nearest(values, ref):
    """For every ref value the index of its nearest entry of values; the match must be one to one."""
    idx = [int(np.argmin(np.abs(values - r))) for r in ref]
    assert len(set(idx)) == len(idx), (values, ref)
    return idx


def compare(tag, bs, nc, Kc, bs_r, nc_r, res_r, bs_abs, nc_rel, sel=None):
    """bs[:k] against bs_r after matching; norming constants / residues of the matched values where sel says so.
    Returns the largest disagreements (bound states absolute, norming constants and residues relative)."""
    k = bs_r.size
    idx = nearest(bs[:k], bs_r)
    e_bs = float(np.abs(bs[idx] - bs_r).max()) if k else 0.0
    e_nc = 0.0
    for i, j in enumerate(idx):
        if sel is not None and not sel[i]:
            continue
        e_nc = max(e_nc, abs(nc[j] - nc_r[i]) / abs(nc_r[i]), abs(nc[Kc + j] - res_r[i]) / abs(res_r[i]))
    print(tag, "K_out", k, "max |bs - ref|", e_bs, "max rel nc/res", e_nc)
    assert e_bs < bs_abs, (tag, e_bs)
    assert e_nc < nc_rel, (tag, e_nc)
    return e_bs, e_nc


# ---- against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disc,D,bsloc", [("2SPLIT4B", 512, SAR), ("2SPLIT3A", 300, SAR), ("4SPLIT4B", 256, SAR),
                                          ("2SPLIT2A", 256, FE)])
def test_vs_oracle(capi, torch, oracle, disc, D, bsloc):
    rcf, bs, nc, kd, st, wn = batched(capi, torch, disc, D, bsloc)
    assert rcf == 0 and not st.any() and not wn.any()
    print(disc, bsloc, "D", D, "roots, Dsub", capi.discspec_search_roots(D, opts_of(disc, bsloc)))
    four = disc.startswith("4SPLIT")
    eps_t = (DC.T[1] - DC.T[0]) / (D - 1)
    for b, (A, c) in enumerate(DC.PAIRS):
        q = DC.signal(D, A, c)
        rc, bs_o, nc_o, res_o = oracle.fnft_nsev_ds(q, DC.T, disc, bsloc=bsloc, bsfilt="FULL", niter=10)
        assert rc == 0
        assert bs_o.size == DC.K_OUT[b] and kd[b] == DC.K_OUT[b], (b, kd[b], bs[b], bs_o)
        _, qp, _, _ = oracle.preprocess(q, eps_t, D, disc)
        _, a_o, _, _ = oracle.scatter_bound_states(qp, DC.T, bs_o, 2 if four else 1, skip_b=True)
        compare("%s %s D=%d signal %d vs oracle" % (disc, bsloc, D, b), bs[b], nc[b], K, bs_o, nc_o, res_o,
                ORACLE_BS_ABS if bsloc == SAR else ORACLE_FE_ABS, ORACLE_NC_REL,
                sel=np.abs(a_o) < 1e-9)     # b = phi/psi is independent of the grid point only at a zero of a


# ---- against the drop-in, signal by signal -------------------------------------------------------------------------------
@pytest.mark.parametrize("disc,D,kw", [("2SPLIT4B", 1024, {}), ("2SPLIT2_MODAL", 1000, {}), ("4SPLIT4B", 512, {}),
                                       ("2SPLIT4B", 4096, {}), ("2SPLIT4B", 1024, {"Dsub": 100})])
def test_vs_drop_in(capi, torch, disc, D, kw):
    n, dsub = capi.discspec_search_roots(D, opts_of(disc, **kw))
    Kc = n                                          # capacity = every root: nothing is truncated on either side
    rcf, bs, nc, kd, st, wn = batched(capi, torch, disc, D, SAR, Kc, **kw)
    assert rcf == 0 and not st.any() and not wn.any()
    q = signals(D)
    worst = [0.0, 0.0]
    for b in range(len(DC.PAIRS)):
        rc, bs_d, nc_d, res_d = capi.fnft_nsev_ds(q[b], DC.T, discretization=disc, bsloc=SAR, K=Kc, **kw)
        assert rc == 0
        assert kd[b] == bs_d.size, (b, kd[b], bs[b, :kd[b]], bs_d)
        e = compare("%s D=%d Dsub=%d roots=%d signal %d vs drop-in" % (disc, D, dsub, n, b), bs[b], nc[b], Kc, bs_d, nc_d,
                    res_d, DROPIN_BS_ABS, DROPIN_NC_REL)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("MEASURED", disc, D, kw, "bound states", worst[0], "norming constants / residues", worst[1])


# ---- options ------------------------------------------------------------------------------------------------------------
def test_dstype_halves_and_null_nc(capi, torch):
    disc, D = "2SPLIT4B", 512
    _, bs, nc, kd, st, _ = batched(capi, torch, disc, D)
    for dstype, lo in (("NORMING_CONSTANTS", 0), ("RESIDUES", K)):
        _, bs1, nc1, kd1, st1, _ = run_plan(capi, torch, signals(D), K, opts_of(disc, discspec_type=dstype))
        assert bs1.tobytes() == bs.tobytes() and np.array_equal(kd1, kd) and not st1.any()
        assert nc1.tobytes() == np.ascontiguousarray(nc[:, lo:lo + K]).tobytes()
    _, bs2, nc2, kd2, st2, _ = run_plan(capi, torch, signals(D), K, opts_of(disc), want_nc=False)
    assert nc2 is None and bs2.tobytes() == bs.tobytes() and np.array_equal(kd2, kd) and not st2.any()


@pytest.mark.parametrize("bsfilt", ["BASIC", "NONE"])
def test_basic_and_none_keep_the_full_result(capi, torch, bsfilt):
    """The oracle itself keeps spurious roots near the real axis under BASIC, so no counts there: with room for every
    root of the subsampled signal (342), every bound state of the FULL result is among the outputs, with its norming
    constant and residue.  NONE keeps every root, refined wherever Newton takes it: 342 values per signal, which may be
    anything (NaN for a root at infinity) except that the FULL result is among them."""
    disc, D = "2SPLIT4B", 512
    Kc = capi.discspec_search_roots(D, opts_of(disc))[0]
    assert Kc == 342
    _, bs_f, nc_f, kd_f, _, _ = batched(capi, torch, disc, D)
    rcf, bs, nc, kd, st, wn = run_plan(capi, torch, signals(D), Kc, opts_of(disc, bound_state_filtering=bsfilt),
                                       finite=bsfilt != "NONE")
    assert not wn.any()
    if bsfilt == "NONE":
        assert (kd == Kc).all()
    else:
        assert not st.any()
    for b in range(len(DC.PAIRS)):
        assert st[b] == 0, (bsfilt, b, st[b])     # none of these pulses has a root with a' = 0 exactly
        live = bs[b, :kd[b]]
        for i, v in enumerate(bs_f[b, :kd_f[b]]):
            dist = np.where(np.isnan(live), np.inf, np.abs(live - v))
            j = int(np.argmin(dist))
            e_nc = max(abs(nc[b, j] - nc_f[b, i]) / abs(nc_f[b, i]),
                       abs(nc[b, Kc + j] - nc_f[b, K + i]) / abs(nc_f[b, K + i]))
            print(bsfilt, "signal", b, "distance to the FULL result", dist[j], "rel nc/res", e_nc)
            assert dist[j] < DROPIN_BS_ABS and e_nc < DROPIN_NC_REL


def test_none_with_room_for_four(capi, torch):
    """NONE with K = 4: four values per signal (the first four roots, refined) and the truncation warning."""
    rcf, bs, nc, kd, st, wn = run_plan(capi, torch, signals(512), 4, opts_of("2SPLIT4B", bound_state_filtering="NONE"),
                                       finite=False)
    assert (kd == 4).all() and (wn & 1).all()


def test_niter_zero_returns_the_subsampled_roots(capi, torch):
    disc, D = "2SPLIT4B", 512
    rcf, bs, nc, kd, st, wn = batched(capi, torch, disc, D, SAR, K, niter=0)
    assert rcf == 0 and not st.any()
    q = signals(D)
    for b in range(len(DC.PAIRS)):
        rc, bs_d, _, _ = capi.fnft_nsev_ds(q[b], DC.T, discretization=disc, bsloc=SAR, niter=0)
        assert rc == 0 and kd[b] == bs_d.size
        idx = nearest(bs[b, :kd[b]], bs_d)
        e = np.abs(bs[b, idx] - bs_d).max()
        print("niter 0 signal", b, "max |bs - drop-in|", e)
        assert e < 1e-6


# ---- slots --------------------------------------------------------------------------------------------------------------
def test_permuted_slots(capi, torch):
    disc, D = "2SPLIT4B", 512
    _, bs, nc, kd, st, _ = batched(capi, torch, disc, D)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    _, bs_p, nc_p, kd_p, st_p, _ = run_plan(capi, torch, signals(D)[perm], K, opts_of(disc))
    assert bs_p.tobytes() == np.ascontiguousarray(bs[perm]).tobytes()
    assert nc_p.tobytes() == np.ascontiguousarray(nc[perm]).tobytes()
    assert np.array_equal(kd_p, kd[perm]) and not st_p.any()


def test_two_calls_and_a_stream(capi, torch):
    disc, D = "2SPLIT4B", 512
    _, bs, nc, kd, _, _ = batched(capi, torch, disc, D)
    s = torch.cuda.Stream()
    _, bs2, nc2, kd2, st2, _ = run_plan(capi, torch, signals(D), K, opts_of(disc), stream=s, calls=2)
    assert bs2.tobytes() == bs.tobytes() and nc2.tobytes() == nc.tobytes() and np.array_equal(kd2, kd) and not st2.any()


def test_failing_modal_slot(capi, torch):
    """A sample with eps_t |q| >= 1 fails the step-size check of 2SPLIT2_MODAL: that slot reports the drop-in's code, the
    others do not notice."""
    disc, D = "2SPLIT2_MODAL", 1000
    _, bs, nc, kd, st, _ = batched(capi, torch, disc, D)
    assert not st.any()
    q = signals(D)
    q[3] = DC.signal(D, 25.0, 0.0)
    code, _, _, _ = capi.fnft_nsev_ds(q[3], DC.T, discretization=disc, bsloc=SAR)
    assert code != 0
    rcf, bs2, nc2, kd2, st2, _ = run_plan(capi, torch, q, K, opts_of(disc))
    assert rcf == code and st2[3] == code
    for b in range(len(DC.PAIRS)):
        if b != 3:
            assert st2[b] == 0 and kd2[b] == kd[b]
            assert bs2[b].tobytes() == bs[b].tobytes() and nc2[b].tobytes() == nc[b].tobytes()


def test_zero_signal_slot(capi, torch):
    disc, D = "2SPLIT4B", 512
    _, bs, nc, kd, _, _ = batched(capi, torch, disc, D)
    q = signals(D)
    q[2] = 0.0
    code, bs_d, _, _ = capi.fnft_nsev_ds(q[2], DC.T, discretization=disc, bsloc=SAR)
    rcf, bs2, nc2, kd2, st2, _ = run_plan(capi, torch, q, K, opts_of(disc))
    assert st2[2] == code and kd2[2] == bs_d.size and rcf == code
    for b in range(len(DC.PAIRS)):
        if b != 2:
            assert st2[b] == 0 and bs2[b].tobytes() == bs[b].tobytes() and nc2[b].tobytes() == nc[b].tobytes()


def test_truncation_to_K(capi, torch):
    disc, D = "2SPLIT4B", 512
    _, bs, _, kd, _, _ = batched(capi, torch, disc, D)
    rcf, bs2, nc2, kd2, st2, wn2 = run_plan(capi, torch, signals(D), 2, opts_of(disc))
    assert rcf == 0 and not st2.any()
    for b in range(len(DC.PAIRS)):
        assert kd2[b] == min(2, kd[b])
        assert (wn2[b] & 1) == (1 if kd[b] > 2 else 0)
        for v in bs2[b, :kd2[b]]:
            assert np.abs(bs[b, :kd[b]] - v).min() < DROPIN_BS_ABS
        if kd2[b] == 2:
            assert abs(bs2[b, 0] - bs2[b, 1]) > 0.1


def test_grid_axis_20000_signals(capi, torch):
    """Signal and workgroup share one grid axis.  Every slot has the count of the pulse it repeats and its values within
    the drop-in bound of the 8-signal plan's (not bitwise: the segments of a sweep depend on the plan's shape)."""
    disc, D, reps = "2SPLIT4B", 128, 2500
    _, bs, nc, kd, st, _ = batched(capi, torch, disc, D)
    assert not st.any() and list(kd) == DC.K_OUT
    rcf, bs2, nc2, kd2, st2, wn2 = run_plan(capi, torch, np.tile(signals(D), (reps, 1)), K, opts_of(disc))
    assert rcf == 0 and not st2.any() and not wn2.any()
    assert np.array_equal(kd2, np.tile(kd, reps))
    worst, worst_nc = 0.0, 0.0
    for b in range(8):
        k = kd[b]
        rows = bs2[b::8, :k]
        order = np.argsort(np.abs(rows[:, :, None] - bs[b, None, None, :k]), axis=1)[:, 0, :]   # nearest entry per reference value
        assert (np.sort(order, axis=1) == np.arange(k)).all()                                  # one to one
        got = np.take_along_axis(rows, order, axis=1)
        worst = max(worst, float(np.abs(got - bs[b, None, :k]).max()))
        for lo in (0, K):       # norming constants, residues of the matched values
            got_nc = np.take_along_axis(nc2[b::8, lo:lo + k], order, axis=1)
            ref_nc = nc[b, None, lo:lo + k]
            worst_nc = max(worst_nc, float((np.abs(got_nc - ref_nc) / np.abs(ref_nc)).max()))
    print("20000 signals: max |bs - 8-signal plan|", worst, "max rel nc/res", worst_nc)
    assert worst < DROPIN_BS_ABS and worst_nc < DROPIN_NC_REL


# ---- call codes ---------------------------------------------------------------------------------------------------------
def test_call_codes(capi, torch):
    D, B = 128, 2
    q = signals(D, DC.PAIRS[:B])
    dq = torch.from_numpy(q.reshape(-1)).to("cuda")
    dbs = torch.zeros(B * K, dtype=torch.complex128, device="cuda")
    dnc = torch.zeros(B * 2 * K, dtype=torch.complex128, device="cuda")
    dk = torch.zeros(B, dtype=torch.int64, device="cuda")
    dg = torch.zeros(B * K, dtype=torch.complex128, device="cuda")
    T = list(DC.T)
    search = capi.DiscSpecSearchPlan(D, K, B, opts_of("2SPLIT4B"))
    guess = capi.DiscSpecPlan(D, K, B, opts_of("2SPLIT4B", "NEWTON"))
    try:
        a = (dq.data_ptr(), T, dbs.data_ptr(), dnc.data_ptr(), dk.data_ptr())
        for i in (0, 1, 2, 4):
            bad = list(a)
            bad[i] = None if i == 1 else 0
            assert search.run_device(*bad) == FNFT_EC_INVALID_ARGUMENT
        assert search.run_device(a[0], [1.0, 1.0], *a[2:]) == FNFT_EC_INVALID_ARGUMENT
        assert search.run_device(a[0], [2.0, 1.0], *a[2:]) == FNFT_EC_INVALID_ARGUMENT
        # a plan of the other kind
        assert capi.DiscSpecPlan.run_device(search, dq.data_ptr(), T, dg.data_ptr(), dbs.data_ptr(), dnc.data_ptr(),
                                            dk.data_ptr()) == -FNFT_EC_INVALID_ARGUMENT
        assert capi.DiscSpecSearchPlan.run_device(guess, *a) == -FNFT_EC_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert not dbs.cpu().numpy().any() and not dnc.cpu().numpy().any() and not dk.cpu().numpy().any()
        w = np.ones(B, np.int32)      # a guess plan has no warnings: all zero, as the header says
        assert guess.L.fnft_amd_discspec_plan_warnings(guess.h, w.ctypes.data_as(ctypes.c_void_p)) == 0
        assert not w.any()
    finally:
        search.close()
        guess.close()
