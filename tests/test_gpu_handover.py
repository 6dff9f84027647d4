"""The tree -> chirp hand-over of the root on the GPU (ChirpParams::root_fused; tests/test_handover_emu.py is the same
in the emulator): every case runs one plan with the hand-over (the default) and one with the switch off
(Plan.set_root_handover), and compares rho, a, b of the two under the bound of the NSE epilogue (chirp_ref.err_bound
with chirp_cases.BOUND_NSE); the small shapes are also compared with the extended-precision reference tests/chirp_ref.py
on the plan's own transfer matrix, as tests/test_gpu_chirp_paths.py does.  After a transform with the hand-over the
exported matrix and its exponent are those of a tree-only plan, signal by signal, and a second transform on the same
plan gives the same bits.  The two large cases are the smallest that reach KChirpColFwd<512> (8 points per lane, LDS):
there the two runs differ in rounding (the tree's own pass takes 16 points per lane), and the oracle would take seconds."""
import numpy as np
import pytest

import chirp_cases as CC
import chirp_ref as R

pytestmark = pytest.mark.gpu


def _c(id, disc, D, M, batch, kappa, n1, ref):
    return dict(CC._c(id, "plan", n1, disc=disc, D=D, M=M, batch=batch, kappa=kappa, cstype="BOTH"), ref=ref)


# N1: the column length of the tree's last split level and of the chirp transform (L = 2N = N1 * 4096)
CASES = [
    _c("modal_2p13_N4_batch3", "2SPLIT2_MODAL", 1 << 13, 1000, 3, 1, 4, True),
    _c("4B_2p14_N16_defocusing", "2SPLIT4B", 1 << 14, 1500, 1, -1, 16, True),
    _c("modal_2p16_N32_M_eq_D_batch2", "2SPLIT2_MODAL", 1 << 16, 1 << 16, 2, 1, 32, True),
    _c("modal_2p20_N512", "2SPLIT2_MODAL", 1 << 20, 1 << 20, 1, 1, 512, False),
    _c("4B_2p19_N512", "2SPLIT4B", 1 << 19, 1 << 19, 1, 1, 512, False),
]
IDS = [c["id"] for c in CASES]


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    c.silence_errors()
    return c


def _transform(capi, c, on, dq, tree_only=False):
    """One plan, one transform (two with the hand-over: the second must repeat the first): dict(out [B, 3M], tm, W,
    names)."""
    import torch
    B, D, M = c["batch"], c["D"], c["M"]
    T, XI = CC.grid(c)
    plan = capi.Plan(D, M, batch=B, discretization=c["disc"])
    assert plan.set_root_handover(on) == 0
    out = torch.zeros(B * 3 * M, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    plan.set_launch_timing(True)
    rc = plan.contspec_device(dq.data_ptr(), 0 if tree_only else out.data_ptr(), T, XI, kappa=c["kappa"])
    assert rc == 0 and plan.finish() == 0, capi.last_error()
    names = [n.replace(" ", "") for n, _ in plan.launch_times()]
    plan.set_launch_timing(False)
    res = out.cpu().numpy()
    if on and not tree_only:
        out.zero_()
        assert plan.contspec_device(dq.data_ptr(), out.data_ptr(), T, XI, kappa=c["kappa"]) == 0 and plan.finish() == 0
        assert np.array_equal(out.cpu().numpy().view(np.float64), res.view(np.float64))
    tms, Ws = [], []
    for b in range(B):
        rc, d, tm, W = plan.transfer_matrix(b)
        assert rc == 0 and d == D * CC.DEG0[c["disc"]]
        tms.append(tm)
        Ws.append(W)
    plan.close()
    return dict(out=res.reshape(B, 3 * M), tm=tms, W=Ws, names=names)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_handover(capi, case):
    import torch
    c = case
    B, D, M = c["batch"], c["D"], c["M"]
    deg1 = CC.DEG0[c["disc"]]
    T, XI = CC.grid(c)
    L = CC.ROW * c["N1"]
    dq = torch.from_numpy(np.concatenate(CC.nse_signals(c, T))).cuda()
    on = _transform(capi, c, True, dq)
    off = _transform(capi, c, False, dq)
    tree = _transform(capi, c, True, dq, tree_only=True)
    # launches: the tree's last inverse column pass is gone from the transform, and nothing finalizes on its own
    inv = "KColInv<%d>" % c["N1"]
    assert inv in off["names"] and inv not in on["names"], (on["names"], off["names"])
    assert "KFinalizeScales" not in on["names"] + off["names"]
    assert [n for n in on["names"] if n != inv] == [n for n in off["names"] if n != inv]
    shifted = c["disc"] in ("2SPLIT2_MODAL", "2SPLIT2A")
    m = CC.out_points(c, M) if c["ref"] else np.array([0, M - 1])   # without the reference: its masses only
    for b in range(B):
        # the root on demand: the matrix and exponent of a plan that never ran the chirp transform
        assert on["W"][b] == tree["W"][b] == off["W"][b]
        assert np.array_equal(on["tm"][b], tree["tm"][b]) and np.array_equal(off["tm"][b], tree["tm"][b])
        ref = R.nsev_epilogue_ref(on["tm"][b], on["W"][b], T, XI, M, D, deg1, shifted, m)
        bound = R.err_bound(CC.BOUND_NSE, L, R.phi(L, *R.nsev_grid(T, XI, M, D, deg1)) + ref["phi_pf"])
        sm = ref["mass"] * ref["scale"]
        x, y = on["out"][b], off["out"][b].astype(R.CLD)
        # hand-over against switch-off at every point; rho in the first-order quotient metric, |H11| = |a| / 2^W
        e = dict(a_ab=R.error(x[M:2 * M], y[M:2 * M], sm), b_ab=R.error(x[2 * M:], y[2 * M:], sm),
                 rho_ab=R.quotient_error(x[:M], y[:M], np.abs(y[M:2 * M]) / ref["scale"], ref["mass"]))
        if c["ref"]:
            for name, r in (("on", on), ("off", off)):
                o = r["out"][b]
                e["rho_" + name] = R.quotient_error(o[m], ref["rho"], ref["H11"], ref["mass"])
                e["a_" + name] = R.error(o[M + m], ref["a"], sm)
                e["b_" + name] = R.error(o[2 * M + m], ref["b"], sm)
        print(c["id"], "signal", b, "bound %.3e" % bound, " ".join("%s %.3e" % kv for kv in sorted(e.items())))
        assert max(e.values()) < bound, (c["id"], b, e, bound)
