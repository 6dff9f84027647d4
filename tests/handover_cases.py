"""Case table of the tree -> chirp hand-over tests (tests/test_gpu_handover.py on the GPU, tests/test_handover_emu.py in
the CPU lane emulator).

The hand-over (ChirpParams::root_fused, chirp_col_fwd_root in nft_kernels.h) is no kernel instantiation of its own: it is
a separate code path inside each KChirpColFwd<N1, false>, N1 = 4 ... 4096, which differ in points per lane, columns per
workgroup, double buffering and whether the row permutation goes through LDS (ChirpColCfg<N1>).  So the table has an
eligible case at every such N1 (tests/test_handover_coverage.py asserts it against the instantiation list),
and the ineligible shapes next to each condition of NftPlan::root_fusable.

A case is a `plan` case of tests/chirp_cases.py (grid, kernels, out_points work on it) with
  tree_n1   column length of the tree's last split level (N = D deg0 = tree_n1 * 2048)
  N1        column length of the chirp transform (L = N1 * 4096)
  eligible  the plan hands the root over (tree_n1 == N1 then)
  why       ineligible cases: the condition of NftPlan::root_fusable that fails, in the words of failing() below
            (N = D deg0; "M > N": the chirp has length 4N; "N not a power of two": the tree pads, N > 2 d;
            "N1 >= kRootFusedMaxN1": the column kernel of that length has no such mode)
  emu       runs in the emulator too (minutes per case there above N1 = 32)
  ref       compared with tests/chirp_ref.py at K output points as well as hand-over on against off (False above
            N1 = 512: the long-double sum takes half a microsecond per term and point, 8 s and more per signal from
            degree 2^21 on; every N1 is compared with the reference on the switched-off path by tests/chirp_cases.py)
  K         output points of the reference (None: 12)
  tree_plan builds the tree-only plan too (False: `tm` and `W` are compared between the on and the off plan only;
            the shapes from N = 2^21 on)
Seconds per case of test_gpu_handover.py::test_handover on an MI355X, the long-double reference included: 2.9
(modal_2p19_N256_defocusing, K = 6, two signals), 2.4 and 2.2 (the two N1 = 512 cases, K = 4), 2.2
(4B_2p16_N64_batch3), 1.9 (4A_2p11_N4_M512_rho: |H11| at all 512 points), 1.5 (4A_2p16_N128_M_eq_N); without
reference 0.2 (4B_2p20_N1024), 0.4 (modal_2p22_N2048), 0.7 (4A_2p21_N4096), 1.3 (4A_2p22_N8192_M512); every other
case below 1 s, the file 20 s.
"""
import numpy as np

import chirp_cases as CC

ROW_TREE = 2048   # kRowTree: N2 of the tree's split levels in the complex symmetric form


def _c(id, disc, D, M, batch, kappa, tree_n1, n1, eligible, cstype="BOTH", emu=False, ref=True, K=None,
       tree_plan=True, why=None):
    assert eligible == (why is None)
    return dict(CC._c(id, "plan", n1, disc=disc, D=D, M=M, batch=batch, kappa=kappa, cstype=cstype, K=K),
                tree_n1=tree_n1, eligible=eligible, emu=emu, ref=ref, tree_plan=tree_plan, why=why)


CASES = [
    # ---- eligible: complex symmetric form, N = D deg0 a power of two, 512 <= M <= N ----
    # N1 = 4: the DIRECT row kernel, a lane holds a whole column (no LDS in the column kernels)
    _c("modal_2p13_N4_batch3", "2SPLIT2_MODAL", 1 << 13, 1000, 3, 1, 4, 4, True, emu=True),
    _c("4B_2p14_N16_defocusing", "2SPLIT4B", 1 << 14, 1500, 1, -1, 16, 16, True, emu=True),
    # N1 = 32: the first column length that goes through LDS; M = D: L = 2N with nothing to spare
    _c("modal_2p16_N32_M_eq_D_batch2", "2SPLIT2_MODAL", 1 << 16, 1 << 16, 2, 1, 32, 32, True, emu=True),
    # the smallest shapes that reach KChirpColFwd<512> (8 points per lane where the tree's own pass takes 16)
    _c("modal_2p20_N512", "2SPLIT2_MODAL", 1 << 20, 1 << 20, 1, 1, 512, 512, True, K=4),
    _c("4B_2p19_N512", "2SPLIT4B", 1 << 19, 1 << 19, 1, 1, 512, 512, True, K=4),
    # deg0 = 4, N = 2^13; M is exactly kRootFusedMinM
    _c("4A_2p11_N4_M512_rho", "2SPLIT4A", 1 << 11, 512, 2, -1, 4, 4, True, cstype="REFLECTION_COEFFICIENT", emu=True),
    _c("2A_2p14_N8_ab", "2SPLIT2A", 1 << 14, 3001, 2, 1, 8, 8, True, cstype="AB", emu=True),
    _c("4B_2p16_N64_batch3", "2SPLIT4B", 1 << 16, 5000, 3, 1, 64, 64, True),
    # M = D deg0 > D: L = 2N with nothing to spare at deg0 > 1
    _c("4A_2p16_N128_M_eq_N", "2SPLIT4A", 1 << 16, 1 << 18, 1, 1, 128, 128, True),
    # kappa = -1 at an LDS column length
    _c("modal_2p19_N256_defocusing", "2SPLIT2_MODAL", 1 << 19, 1000, 2, -1, 256, 256, True, K=6),
    _c("4B_2p20_N1024", "2SPLIT4B", 1 << 20, 4001, 1, 1, 1024, 1024, True, ref=False, K=6, tree_plan=False),
    _c("modal_2p22_N2048", "2SPLIT2_MODAL", 1 << 22, 1000, 1, 1, 2048, 2048, True, ref=False, K=4, tree_plan=False),
    # N = 2^23: the last length that has the mode
    _c("4A_2p21_N4096", "2SPLIT4A", 1 << 21, 600, 1, 1, 4096, 4096, True, ref=False, K=4, tree_plan=False),
    # ---- not eligible: the same launches, and bitwise the same outputs, whichever way the switch is ----
    # one below the cut: the launches of modal_2p13_N4_batch3 with the switch off
    _c("modal_2p13_M511", "2SPLIT2_MODAL", 1 << 13, 511, 3, 1, 4, 4, False, emu=True, why="M < kRootFusedMinM"),
    _c("modal_2p13_M20000_L4N", "2SPLIT2_MODAL", 1 << 13, 20000, 1, 1, 4, 8, False, emu=True, why="M > N"),
    _c("modal_D12000_padded", "2SPLIT2_MODAL", 12000, 1000, 1, 1, 8, 4, False, emu=True, why="N not a power of two"),
    # deg0 = 3: N = 3 * 2^12 is no power of two, the tree pads its transforms (N > 2 d)
    _c("3A_D4096_deg3", "2SPLIT3A", 1 << 12, 1000, 1, 1, 8, 4, False, why="N not a power of two"),
    # N = 2^24, the tree of tree_cases.plan_4A_D4194304_max, with M at the cut: KChirpColFwd<8192> has no such mode, a
    # wrong G.N1 < kRootFusedMaxN1 guard would hand it a root all the same
    _c("4A_2p22_N8192_M512", "2SPLIT4A", 1 << 22, 512, 1, 1, 8192, 8192, False, ref=False, K=4, tree_plan=False,
       why="N1 >= kRootFusedMaxN1"),
]

# KChirpColFwd<n, false> that cannot take a root, with the reason (test_handover_coverage)
EXCLUDED = {
    2: "no split level of the tree has two rows (N = 2 * 2048 is a fused level)",
    8192: "kRootFusedMaxN1: 16 points per lane leave no registers for the mode",
}

CSLEN = {"REFLECTION_COEFFICIENT": 1, "AB": 2, "BOTH": 3}
DEG0 = CC.DEG0
MIN_M = 512       # NftPlan::kRootFusedMinM
MAX_N1 = 8192     # kRootFusedMaxN1


def case(id):
    return next(c for c in CASES if c["id"] == id)


def ids(cases):
    return [c["id"] for c in cases]


grid = CC.grid   # (T, XI) of a case: the tight grid of chirp_cases (Phi ~ log2 L)


def failing(c):
    """The conditions of NftPlan::root_fusable that the numbers of a case fail (empty: eligible), as `why` names them."""
    N = c["D"] * DEG0[c["disc"]]
    out = set()
    if N & (N - 1):
        out.add("N not a power of two")
    if c["M"] < MIN_M:
        out.add("M < kRootFusedMinM")
    if c["M"] > N:
        out.add("M > N")
    if N >= MAX_N1 * ROW_TREE:
        out.add("N1 >= kRootFusedMaxN1")
    return out


def flipped(c):
    """An ineligible case with the one thing changed that its `why` names, everything else kept: that shape is eligible
    (tests/test_handover_coverage.py watches the schedule change)."""
    N = c["D"] * DEG0[c["disc"]]
    if c["why"] == "M < kRootFusedMinM":
        return dict(c, M=MIN_M)
    if c["why"] == "M > N":
        return dict(c, M=N)
    if c["why"] == "N1 >= kRootFusedMaxN1":
        return dict(c, D=c["D"] // 2)
    # as many coefficients as the next power of two holds (no deg0 = 3 scheme has such a D: one step per sample)
    return dict(c, D=1 << (N - 1).bit_length(), disc="2SPLIT2_MODAL")


# Signals.  chirp_cases.nse_signals keeps every pulse within a factor of two; then the maxima of every signal's root lie
# in one binade, the scale KChirpRows applies is the same power of two for all of them and a wrong signal index or a
# stale maximum changes nothing.  A smooth pulse cannot change that however strong it is: the largest coefficient of
# the matrix is its leading one, the product of the steps' norms (1 + kappa |q eps_t|^2)^(-1/2), which stays at 1 while
# sum |q eps_t|^2 is small.  So every signal is the smooth pulse of nse_signals plus SPIKES[slot] single samples with
# |q| eps_t = theta(c) at random places: each divides (kappa = 1) or multiplies (kappa = -1) the leading coefficient by a
# fixed factor, 0.78 or 1.67, so the slots' exponents differ -- test_handover asserts it -- and the peak amplitudes differ
# by theta D / 2 >= 800.  A few spikes add a few coefficients only: the values stay of the order of the mass sum |c_n|
# that the metric divides by, as with the smooth pulses, where a signal of noise would put sqrt(N) between the two.
# 2SPLIT4B's steps are not unitary and its coefficients hardly move at 0.8 (6 spikes: W stays -1); focusing, where |q|
# eps_t may exceed 1, its spikes are 2.0 high (W = 1, -1, 0 for 6, 0, 3 spikes in the emulator at N1 = 4).
SPIKES = (6, 0, 3)


def theta(c):
    return 2.0 if c["disc"] == "2SPLIT4B" and c["kappa"] == 1 else 0.8


def signals(c, T, which="A"):
    """`batch` signals of D samples.  which = "B": another set on the same grid, 64 times smaller -- other pulses
    (nse_signals with salt 1), the spike counts of "A" moved on by one slot, the spikes at other places, everything
    divided by 64.  Its spikes are too low to move W: a small set after a large one, the order in which a stale
    maximum (atomic max) or exponent would show."""
    D, B = c["D"], c["batch"]
    eps_t = (T[1] - T[0]) / (D - 1)
    r = CC.rng(c, 7 if which == "A" else 8)
    out = []
    for k, q in enumerate(CC.nse_signals(c, T, salt=0 if which == "A" else 1)):
        n = SPIKES[k] if which == "A" else SPIKES[(k + 1) % B]
        at = r.choice(D, size=n, replace=False)
        q[at] += theta(c) / eps_t * np.exp(1j * r.uniform(0.0, 2.0 * np.pi, n))
        out.append(q if which == "A" else q / 64.0)
    return out


def other_xi(XI):
    """A second grid of the same number of points and another width: the filter spectrum's key misses."""
    return (XI[0], XI[0] + 1.5 * (XI[1] - XI[0]))


def split(c, out):
    """(rho, a, b) of one signal's output in the layout of its contspec type (None where the type has no such part)."""
    M = c["M"]
    t = c["cstype"]
    rho = out[:M] if t != "AB" else None
    o = M if t == "BOTH" else 0
    a, b = (out[o:o + M], out[o + M:o + 2 * M]) if t != "REFLECTION_COEFFICIENT" else (None, None)
    return rho, a, b


def reference(c, tm, W, T, XI, m=None):
    """What errors() measures one signal against: the extended-precision epilogue (chirp_ref.nsev_epilogue_ref) of the
    transfer matrix tm, exponent W, at the output points m, with the masses of the metric and the bound --
    chirp_ref.err_bound with chirp_cases.BOUND_NSE.  m = None: masses and bound only (no polynomial is evaluated: the
    mass is sum |c_n| |A|^-n as chirp_ref.chirpz_ref forms it)."""
    import chirp_ref as R
    D, M = c["D"], c["M"]
    deg1 = DEG0[c["disc"]]
    L = CC.ROW * c["N1"]
    A, V = R.nsev_grid(T, XI, M, D, deg1)
    shifted = c["disc"] in ("2SPLIT2_MODAL", "2SPLIT2A")
    if m is not None:
        ref = R.nsev_epilogue_ref(tm, W, T, XI, M, D, deg1, shifted, m)
    else:
        la = R.ld_log(A)[0]
        w = np.exp(-np.arange(tm.shape[1], dtype=R.LD)[::-1] * la)   # highest power first, as chirpz_ref reverses it
        xi, pf_rho, pf_a, pf_b = R.nsev_phase_factors(T, XI, M, D, deg1, shifted, np.array([0, M - 1]))
        ref = dict(mass=max(np.sum(np.abs(tm[0]).astype(R.LD) * w), np.sum(np.abs(tm[2]).astype(R.LD) * w)),
                   scale=np.ldexp(R.LD(1), int(W)),
                   phi_pf=float(np.max(np.abs(xi)) * max(abs(pf_rho), abs(pf_a), abs(pf_b))))
    ref["bound"] = R.err_bound(CC.BOUND_NSE, L, R.phi(L, A, V) + ref["phi_pf"])
    if c["cstype"] == "REFLECTION_COEFFICIENT":
        # no a in this type: |H11| at every point from the reference (cheap at the one small shape that asks)
        ref["H11_all"], _ = R.chirpz_ref(tm[0], A, V, np.arange(M))
    return ref


def errors(c, out, other, ref, m=None):
    """Mass-relative errors of one signal's output `out` under the metric of the NSE epilogue: against `other` (the run
    with the switch the other way) at every point -- keys *_ab -- and, m given, against reference(..., m) at the output
    points m -- keys rho, a, b.  rho is measured in the first-order quotient metric, whose |H11| comes from the
    reference, and from |a| / 2^W of `other` at every point where the type has a."""
    import chirp_ref as R
    sm = ref["mass"] * ref["scale"]
    rho, a, b = split(c, out)
    rho2, a2, b2 = split(c, other)
    e = {}
    if a is not None:
        e["a_ab"] = R.error(a, a2.astype(R.CLD), sm)
        e["b_ab"] = R.error(b, b2.astype(R.CLD), sm)
        if m is not None:
            e["a"] = R.error(a[m], ref["a"], sm)
            e["b"] = R.error(b[m], ref["b"], sm)
    if rho is not None:
        den = np.abs(a2) / ref["scale"] if a is not None else ref["H11_all"]
        e["rho_ab"] = R.quotient_error(rho, rho2.astype(R.CLD), den, ref["mass"])
        if m is not None:
            e["rho"] = R.quotient_error(rho[m], ref["rho"], ref["H11"], ref["mass"])
    return e
