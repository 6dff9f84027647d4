"""The tree -> chirp hand-over of the root on the GPU (ChirpParams::root_fused; tests/test_handover_emu.py is the same
in the emulator).  The cases are those of tests/handover_cases.py: an eligible one at every column length N1 = 4 ... 4096
of KChirpColFwd<N1, false> -- the hand-over is a code path of its own inside each -- and the ineligible shapes.

test_handover runs one plan with the hand-over (the default) and one with the switch off (Plan.set_root_handover), and
compares rho, a, b of the two under the bound of the NSE epilogue (chirp_ref.err_bound with chirp_cases.BOUND_NSE); the
cases marked `ref` are also compared with the extended-precision reference tests/chirp_ref.py on the plan's own
transfer matrix, as tests/test_gpu_chirp_paths.py does.  After a transform with the hand-over the exported matrix and
its exponent are those of a tree-only plan, signal by signal, and a second transform on the same plan gives the same
bits.  An ineligible case launches the same kernels and gives the same bits whichever way the switch is.

The other tests are the call sequences that leave a root pending (NftPlan::root_pending, final_pending) and every
reader that must resolve it (ensure_root): what one plan gives after such a sequence is, bit for bit, what a fresh plan
gives for the same input in a single call.

Largest measured error over bound per form: profiles/handover_err.json (written through FNFT_HANDOVER_ERR_JSON)."""
import json
import os

import numpy as np
import pytest

import chirp_cases as CC
import handover_cases as HC

pytestmark = pytest.mark.gpu

IDS = HC.ids(HC.CASES)
# the shapes of the call sequences: a lane holds a whole column (N1 = 4); the column goes through LDS (N1 = 32)
SEQ = [HC.case("modal_2p13_N4_batch3"), HC.case("modal_2p16_N32_M_eq_D_batch2")]
SEQ_IDS = HC.ids(SEQ)

_measured = {}


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    c.silence_errors()
    yield c
    out = os.environ.get("FNFT_HANDOVER_ERR_JSON")   # optional record of the measured errors
    if out:
        with open(out, "w") as f:
            json.dump(_measured, f, indent=1)


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.float64), np.ascontiguousarray(y).view(np.float64))


class _Plan:
    """One plan of a case and the calls the tests make on it; every call waits for its result."""

    def __init__(self, capi, c, on=True):
        self.capi, self.c = capi, c
        self.plan = capi.Plan(c["D"], c["M"], batch=c["batch"], discretization=c["disc"])
        assert self.plan.set_root_handover(on) == 0
        self.T, self.XI = HC.grid(c)
        self.cl = HC.CSLEN[c["cstype"]] * c["M"]
        self.deg = c["D"] * HC.DEG0[c["disc"]]

    def switch(self, on):
        assert self.plan.set_root_handover(on) == 0

    def enqueue(self, dq, out, XI=None, stream=0):
        rc = self.plan.contspec_device(dq.data_ptr(), out.data_ptr() if out is not None else 0, self.T, XI or self.XI,
                                       kappa=self.c["kappa"], contspec_type=self.c["cstype"], stream=stream)
        assert rc == 0, self.capi.last_error()

    def transform(self, dq, XI=None, tree_only=False):
        """One transform of the signals dq (device tensor): (out [B, cl], launches); tree_only: no output."""
        import torch
        out = None if tree_only else torch.zeros(self.c["batch"] * self.cl, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        self.plan.set_launch_timing(True)
        self.enqueue(dq, out, XI)
        assert self.plan.finish() == 0, self.capi.last_error()
        names = self.names()
        self.plan.set_launch_timing(False)
        return (None if tree_only else out.cpu().numpy().reshape(self.c["batch"], self.cl)), names

    def names(self):
        return [n.replace(" ", "") for n, _ in self.plan.launch_times()]

    def from_tm(self, dtm, W):
        import torch
        out = torch.zeros(self.c["batch"] * self.cl, dtype=torch.complex128, device="cuda")
        rc = self.plan.contspec_from_tm_device(dtm.data_ptr(), W, out.data_ptr(), self.T, self.XI,
                                               contspec_type=self.c["cstype"])
        assert rc == 0 and self.plan.finish() == 0, self.capi.last_error()
        return out.cpu().numpy().reshape(self.c["batch"], self.cl)

    def matrix(self, b, device=False):
        """(tm [4, deg + 1], W) of signal b through the host or the device export."""
        if not device:
            rc, d, tm, W = self.plan.transfer_matrix(b)
            assert rc == 0 and d == self.deg, self.capi.last_error()
            return tm, W
        import torch
        buf = torch.zeros(4 * (self.deg + 1), dtype=torch.complex128, device="cuda")
        rc, d, W = self.plan.transfer_matrix_device(buf.data_ptr(), b)
        assert rc == 0 and d == self.deg, self.capi.last_error()
        return buf.cpu().numpy().reshape(4, self.deg + 1), W

    def matrices(self):
        return [self.matrix(b) for b in range(self.c["batch"])]

    def close(self):
        self.plan.close()


def _dev(sig):
    import torch
    return torch.from_numpy(np.concatenate(sig)).cuda()


def _same_matrices(x, y):
    return len(x) == len(y) and all(wx == wy and _same(tx, ty) for (tx, wx), (ty, wy) in zip(x, y))


# ---- values at every case ------------------------------------------------------------------------------------------
def _run(capi, c, on, dq, tree_only=False):
    """One plan, one transform (two with the hand-over: the second must repeat the first): dict(out, tm, names)."""
    p = _Plan(capi, c, on)
    out, names = p.transform(dq, tree_only=tree_only)
    if on and not tree_only:
        again, _ = p.transform(dq)
        assert _same(again, out)
    tm = p.matrices()
    p.close()
    return dict(out=out, tm=tm, names=names)


@pytest.mark.parametrize("case", HC.CASES, ids=IDS)
def test_handover(capi, case):
    c = case
    B, M = c["batch"], c["M"]
    T, XI = HC.grid(c)
    dq = _dev(HC.signals(c, T))
    on = _run(capi, c, True, dq)
    off = _run(capi, c, False, dq)
    inv = "KColInv<%d>" % c["tree_n1"]
    assert "KFinalizeScales" not in on["names"] + off["names"]
    assert inv in off["names"]
    if c["eligible"]:
        # launches: the tree's last inverse column pass is gone from the transform, and nothing finalizes on its own
        assert inv not in on["names"], on["names"]
        assert [n for n in on["names"] if n != inv] == [n for n in off["names"] if n != inv]
    else:
        assert on["names"] == off["names"]
        assert _same(on["out"], off["out"])
    # the root on demand: the matrix and exponent of a plan that never ran the chirp transform
    assert _same_matrices(on["tm"], off["tm"])
    if c["tree_plan"]:
        assert _same_matrices(on["tm"], _run(capi, c, True, dq, tree_only=True)["tm"])
    W = [w for _, w in on["tm"]]
    if B > 1:
        # the signals' roots lie in different binades: the scale KChirpRows applies differs from signal to signal
        assert len(set(W)) == B and any(W), W
    m = CC.out_points(c, M) if c["ref"] else None
    for b in range(B):
        tm = on["tm"][b][0]
        # hand-over against switch-off at every point (rho in the first-order quotient metric, |H11| = |a| / 2^W), and
        # both runs against the reference at the K points
        ref = HC.reference(c, tm, W[b], T, XI, m)
        rec = dict(bound=ref["bound"], W=W[b], **HC.errors(c, on["out"][b], off["out"][b], ref))
        if c["ref"]:
            for name, r in (("on", on), ("off", off)):
                er = HC.errors(c, r["out"][b], r["out"][b], ref, m)
                rec.update({k + "_" + name: v for k, v in er.items() if not k.endswith("_ab")})
        _measured["%s[b=%d]" % (c["id"], b)] = rec
        print(c["id"], "signal", b, " ".join("%s %.3e" % kv for kv in sorted(rec.items())))
        worst = max(v for k, v in rec.items() if k not in ("bound", "W"))
        assert worst < ref["bound"], (c["id"], b, rec)


# ---- every reader of a pending root --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh(capi):
    """What a fresh plan gives in a single call, computed once per (case, signal set, grid, switch): dict(out, tm,
    names).  grid "other": handover_cases.other_xi."""
    memo = {}

    def get(c, which="A", grid="case", on=True):
        key = (c["id"], which, grid, on)
        if key not in memo:
            p = _Plan(capi, c, on)
            out, names = p.transform(_dev(HC.signals(c, p.T, which)), HC.other_xi(p.XI) if grid == "other" else None)
            memo[key] = dict(out=out, names=names, tm=p.matrices())
            p.close()
        return memo[key]
    return get


@pytest.mark.parametrize("case", SEQ, ids=SEQ_IDS)
def test_another_signal_on_the_same_plan(capi, fresh, case):
    """Set A, then set B on the same grids (the filter spectrum comes from the cache, v_mode 2: the column kernel's
    narrower grid), then B on another XI (a miss: the filter job's wider grid runs over chirp_col_fwd_root's early
    return), then A again: each output, and the matrices exported at the end, are a fresh plan's -- no maximum (max2_out, filled by
    atomic max), exponent (fin_wexp, updated in place by KChirpRows) or scale survives a call."""
    c = case
    p = _Plan(capi, c)
    qA, qB = _dev(HC.signals(c, p.T)), _dev(HC.signals(c, p.T, "B"))
    WA, WB = ([w for _, w in fresh(c, s)["tm"]] for s in "AB")
    assert WA != WB, (WA, WB)   # the exponents of the two sets differ (B's spikes are too low to move W)
    inv = "KColInv<%d>" % c["tree_n1"]
    # ... and the large set once more after the small one (a miss again: the key is the other grid's)
    for which, dq, grid in (("A", qA, "case"), ("B", qB, "case"), ("B", qB, "other"), ("A", qA, "case")):
        out, names = p.transform(dq, HC.other_xi(p.XI) if grid == "other" else None)
        assert inv not in names
        assert _same(out, fresh(c, which, grid)["out"]), (which, grid)
    assert _same_matrices(p.matrices(), fresh(c)["tm"])
    p.close()


@pytest.mark.parametrize("case", SEQ, ids=SEQ_IDS)
def test_export_variants(capi, fresh, case):
    """After a transform with the hand-over: the device export for b descending, then the host export ascending.  The
    tree's last pass runs once, nothing finalizes a second time, every matrix is the tree-only plan's."""
    import torch
    c = case
    p = _Plan(capi, c)
    dq = _dev(HC.signals(c, p.T))
    t = _Plan(capi, c)
    t.transform(dq, tree_only=True)
    tree = t.matrices()
    t.close()
    out = torch.zeros(c["batch"] * p.cl, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    p.plan.set_launch_timing(True)
    p.enqueue(dq, out)
    assert p.plan.finish() == 0
    got = [p.matrix(b, device=True) for b in reversed(range(c["batch"]))][::-1]
    assert _same_matrices(got, tree)
    assert _same_matrices(p.matrices(), tree)
    torch.cuda.synchronize()
    names = p.names()
    assert names.count("KColInv<%d>" % c["tree_n1"]) == 1 and "KFinalizeScales" not in names, names
    assert names.count("KExportTm") == 2 * c["batch"], names
    assert _same(out.cpu().numpy().reshape(c["batch"], p.cl), fresh(c)["out"])
    assert _same_matrices(tree, fresh(c)["tm"])
    p.close()


@pytest.mark.parametrize("case", SEQ, ids=SEQ_IDS)
def test_callers_matrix_in_between(capi, fresh, case):
    """A transform with the hand-over, then contspec_from_tm_device on another signal set's matrices with W = 7, then
    the export: the from-tm output is a fresh plan's, and the exported matrices are the first set's -- the kept scratch
    (root_G.Z) and the pending root survive a chirp run that does not consume them."""
    import torch
    c = case
    tmB = np.stack([tm for tm, _ in fresh(c, "B")["tm"]])
    dtm = torch.from_numpy(tmB.reshape(-1)).cuda()
    f = _Plan(capi, c)
    alone = f.from_tm(dtm, 7)
    f.close()
    assert np.any(alone != 0)
    p = _Plan(capi, c)
    out, _ = p.transform(_dev(HC.signals(c, p.T)))
    assert _same(out, fresh(c)["out"])
    assert _same(p.from_tm(dtm, 7), alone)
    p.plan.set_launch_timing(True)
    assert _same_matrices(p.matrices(), fresh(c)["tm"])
    names = p.names()
    assert names.count("KColInv<%d>" % c["tree_n1"]) == 1 and "KFinalizeScales" not in names, names
    p.close()


@pytest.mark.parametrize("case", SEQ, ids=SEQ_IDS)
def test_tree_only_then_transform(capi, fresh, case):
    """contspec_device without an output and the export: ensure_root resolves the pending root AND the pending finalize.
    Then a full transform of another signal set on the same plan: outputs and matrices are a fresh plan's."""
    c = case
    p = _Plan(capi, c)
    p.plan.set_launch_timing(True)
    p.enqueue(_dev(HC.signals(c, p.T)), None)
    assert p.plan.finish() == 0
    assert _same_matrices(p.matrices(), fresh(c)["tm"])
    names = p.names()
    assert names.count("KColInv<%d>" % c["tree_n1"]) == 1 and names.count("KFinalizeScales") == 1, names
    out, names = p.transform(_dev(HC.signals(c, p.T, "B")))
    assert names == fresh(c, "B")["names"]
    assert _same(out, fresh(c, "B")["out"])
    assert _same_matrices(p.matrices(), fresh(c, "B")["tm"])
    p.close()


@pytest.mark.parametrize("case", SEQ, ids=SEQ_IDS)
def test_switch_toggled_on_one_plan(capi, fresh, case):
    """On, off, on again on one plan: calls 1 and 3 give the same bits, call 2 those of a plan that always had the
    switch off; the tree's last pass is launched in call 2 only."""
    c = case
    p = _Plan(capi, c)
    dq = _dev(HC.signals(c, p.T))
    inv = "KColInv<%d>" % c["tree_n1"]
    res = []
    for on in (True, False, True):
        p.switch(on)
        res.append(p.transform(dq))
    assert [inv in names for _, names in res] == [False, True, False]
    assert _same(res[0][0], res[2][0]) and _same(res[0][0], fresh(c)["out"])
    assert _same(res[1][0], fresh(c, on=False)["out"])
    assert res[1][1] == fresh(c, on=False)["names"] and res[2][1] == fresh(c)["names"]
    assert _same_matrices(p.matrices(), fresh(c)["tm"])
    p.close()


def test_two_handover_plans_two_streams(capi, fresh):
    """Two eligible plans of different column lengths, each on its own stream, transforms of two signal sets in flight
    without synchronisation in between (the pattern of test_gpu_parity.py::test_two_plans_two_streams_in_flight): every
    result is bit for bit the one a fresh plan gives alone on the default stream."""
    import torch
    plans = [_Plan(capi, c) for c in SEQ]
    streams = [torch.cuda.Stream() for _ in SEQ]
    sig = [[_dev(HC.signals(p.c, p.T, w)) for w in "AB"] for p in plans]
    outs = [[torch.zeros(p.c["batch"] * p.cl, dtype=torch.complex128, device="cuda") for _ in "AB"] for p in plans]
    torch.cuda.synchronize()
    for rep in range(2):
        for k in range(2):                                   # both streams busy at once, no host synchronisation
            for i, p in enumerate(plans):
                p.enqueue(sig[i][k], outs[i][k], stream=streams[i].cuda_stream)
    torch.cuda.synchronize()
    for i, p in enumerate(plans):
        assert p.plan.finish(streams[i].cuda_stream) == 0, capi.last_error()
        for k, w in enumerate("AB"):
            assert _same(outs[i][k].cpu().numpy().reshape(p.c["batch"], p.cl), fresh(p.c, w)["out"]), (p.c["id"], w)
        assert _same_matrices(p.matrices(), fresh(p.c, "B")["tm"])
        p.close()
