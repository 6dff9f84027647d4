"""The Darboux path tests without a GPU: that the long-double reference of tests/darboux_ref.py is sound (two
independent algorithms for the multi-soliton, closed forms, the same integrator in mpmath at 45 digits), that the
yardsticks which set the GPU bound (tests/darboux_cases.py) stay below a cap, that the bound separates a result with one
norming constant off by 1e-11 from a right one, the recorded distance of the reference's skipped step at ks == 0, and the
coverage of the case table."""
import numpy as np
import pytest

import darboux_cases as DC
import darboux_ref as R
from test_emu_kernels import emu, kernel_list  # noqa: F401  (module fixture: builds and loads tests/emu/libfnft_emu.so)

U = R.U
CAP = 4000 * U
MODE0 = [c for c in DC.CASES if c["mode"] == 0]
MODE1 = [c for c in DC.CASES if c["mode"] == 1]
LD = np.longdouble


# ---- soundness of the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MODE0, ids=DC.case_ids(MODE0))
def test_recursion_and_darboux_steps_on_zero_agree(case):
    """solitons_ref and cdt_exact_zero_seed_ref, two algorithms that share only the inputs, within 0.5 u (measured: at
    most 0.033 u, K32_wide).  Clustered bound states (spaced 0.1 apart) give 350 to 700 u here: such a case has no
    place in the table, because its reference would not be known to the accuracy the bound needs."""
    bs, nc = R.prepared(case["bs"], case["nc"], case["dstype"] == DC.RESIDUES)
    q = R.cdt_exact_zero_seed_ref(bs, nc, case["T"], case["D"])
    err = R.error(q, DC.evaluated(case)["q_ref"])
    assert err <= 0.5 * U, (case["id"], err / U)


def test_one_soliton_closed_form():
    """K = 1: q = -2 eta exp(-i (2 xi t + arg b)) sech(2 eta t - ln |b|), lambda = xi + i eta."""
    c = DC.BY_ID["K1"]
    _, t, _ = R.grid(c["T"], c["D"])
    l, b = complex(c["bs"][0]), np.clongdouble(c["nc"][0])
    xi, eta = LD(l.real), LD(l.imag)
    q = -2 * eta * np.exp(-1j * (2 * xi * t + np.arctan2(b.imag, b.real))) / np.cosh(2 * eta * t - np.log(np.abs(b)))
    err = R.error(DC.evaluated(c)["q_ref"], q)
    assert err <= 0.1 * U, err / U


def test_five_solitons_are_5_sech():
    """The reference's multisoliton_cdt: bound states 0.5i .. 4.5i with norming constants -+1 are 5 sech(t)."""
    c = DC.BY_ID["K5_sech"]
    _, t, _ = R.grid(c["T"], c["D"])
    err = R.error(DC.evaluated(c)["q_ref"], 5 / np.cosh(t))
    assert err <= 0.1 * U, err / U


def _mp_cdt(c, dps=45):
    """cdt_ref restated in mpmath: the same sort, conversion, half-step integrator (limit at ks == 0) and Darboux steps."""
    import mpmath as mp
    with mp.workdps(dps):
        cv = lambda z: mp.mpc(float(z.real), float(z.imag))    # noqa: E731  (doubles convert exactly)
        bsd, ncd = R.sort_bound_states(np.asarray(c["bs"], np.complex128), np.asarray(c["nc"], np.complex128))
        bs, nc = [cv(z) for z in bsd], [cv(z) for z in ncd]
        K, D, T = len(bs), c["D"], c["T"]
        if c["dstype"] == DC.RESIDUES:
            out = []
            for i in range(K):
                tmp = mp.mpc(1)
                for j in range(K):
                    if j != i:
                        tmp = tmp * (bs[i] - bs[j]) / (bs[i] - mp.conj(bs[j]))
                out.append(nc[i] / (2j * bs[i].imag) * tmp)
            nc = out
        q = [cv(z) for z in DC.seed_samples(c)]
        h = mp.mpf((T[1] - T[0]) / (D - 1)) / 2
        phi, psi = [], []
        for l in bs:
            st = []
            for x in q:
                ks = -(x.real * x.real + x.imag * x.imag) - l * l
                if ks == 0:
                    ch, sh = mp.mpc(1), mp.mpc(h)
                else:
                    k = mp.sqrt(ks)
                    ch, sh = mp.cosh(k * h), mp.sinh(k * h) / k
                st.append((ch - 1j * l * sh, x * sh, -mp.conj(x) * sh, ch + 1j * l * sh))
            p = (mp.exp(-1j * l * mp.mpf(T[0])), mp.mpc(0))
            ph = [p]
            for n in range(1, D):
                for m in (n - 1, n):
                    a, b, cc, d = st[m]
                    p = (a * p[0] + b * p[1], cc * p[0] + d * p[1])
                ph.append(p)
            s = (mp.mpc(0), mp.exp(1j * l * mp.mpf(T[1])))
            ps = [None] * D
            ps[D - 1] = s
            for n in range(D - 1, 0, -1):
                for m in (n, n - 1):
                    a, b, cc, d = st[m]
                    s = (d * s[0] - b * s[1], -cc * s[0] + a * s[1])
                ps[n - 1] = s
            phi.append(ph)
            psi.append(ps)
        res = np.zeros(D, np.clongdouble)
        for n in range(D):
            qn = q[n]
            S1, S2 = [], []
            for i in range(K):
                p1, p2 = phi[i][n]
                s1, s2 = psi[i][n]
                for j in range(i):
                    a, ac, b = bs[i] - S1[j], bs[i] - mp.conj(S1[j]), S2[j]
                    p1, p2 = a * p1 - b * p2, mp.conj(b) * p1 + ac * p2
                    s1, s2 = a * s1 - b * s2, mp.conj(b) * s1 + ac * s2
                beta = (p1 - nc[i] * s1) / (p2 - nc[i] * s2)
                ab = beta.real * beta.real + beta.imag * beta.imag
                S1.append((ab * bs[i] + mp.conj(bs[i])) / (1 + ab))
                S2.append(2j * bs[i].imag * beta / (1 + ab))
                qn = qn - 2j * S2[i]
            res[n] = LD(mp.nstr(qn.real, 30)) + 1j * LD(mp.nstr(qn.imag, 30))
        return res


_MP = [c for c in MODE1 if c["D"] <= 512]


@pytest.mark.parametrize("case", _MP, ids=DC.case_ids(_MP))
def test_reference_agrees_with_mpmath(case):
    """cdt_ref in long double within 1 u of the same algorithm at 45 digits (measured: 0.02 to 0.2 u)."""
    err = R.error(DC.evaluated(case)["q_ref"], _mp_cdt(case))
    print("%s: %.3f u" % (case["id"], err / U))
    assert err <= 1.0 * U, (case["id"], err / U)


@pytest.mark.parametrize("cid", ("chirp_K4_D10", "chirp_K4_D300", "chirp_K2_D2050", "ks_zero_K2"))
def test_chunked_association_is_the_same_function(cid):
    """The chunked eigenfunctions of the second yardstick, run in long double, reproduce the sequential reference: what
    e2 measures is the rounding of that association, not another function."""
    c = DC.BY_ID[cid]
    bs, nc = R.prepared(c["bs"], c["nc"], c["dstype"] == DC.RESIDUES)
    q = DC.seed_samples(c)
    with np.errstate(over="ignore", invalid="ignore"):
        phi, psi = R.eigenfunctions_chunked(bs, q, c["T"], np.clongdouble)
    err = R.error(R.cdt_steps(bs, nc, q, phi, psi), DC.evaluated(c)["q_ref"])
    assert err <= 0.5 * U, (cid, err / U)


def test_grid_and_zero_crossing():
    """zc as the host computes it: 0 where every sample is right of 0 and where none is; t = 0 on a grid point for the
    odd sizes on a symmetric window."""
    assert R.grid(DC.BY_ID["K4_right"]["T"], 200)[2] == 0
    assert R.grid(DC.BY_ID["K4_left"]["T"], 200)[2] == 0
    for cid, n0 in (("K3_hugeb", 128), ("K2_bigT", 500), ("K2_D3", 1), ("K2_D513", 256)):
        c = DC.BY_ID[cid]
        eps, t, zc = R.grid(c["T"], c["D"])
        assert zc == n0 and c["T"][0] + eps * n0 == 0.0, (cid, zc)
    assert R.grid((-12.0, 12.0), 256)[2] == 128


def test_sort_is_the_references_exchange_sort():
    """Descending imaginary part; the constants travel with their bound states; K16_wide has equal imaginary parts, so
    the order among them is the exchange sort's, not that of a stable sort."""
    c = DC.BY_ID["K16_wide"]
    bs, nc = R.sort_bound_states(c["bs"], c["nc"])
    assert np.all(np.diff(bs.imag) <= 0)
    pairs = {(complex(a), complex(b)) for a, b in zip(c["bs"], c["nc"])}
    assert {(complex(a), complex(b)) for a, b in zip(bs, nc)} == pairs
    stable = c["bs"][np.argsort(-c["bs"].imag, kind="stable")]
    assert not np.array_equal(bs, stable)
    u = DC.BY_ID["K4_unsorted"]
    assert np.array_equal(R.sort_bound_states(u["bs"], u["nc"])[0], DC.K4_BS) and not np.array_equal(u["bs"], DC.K4_BS)


# ---- the yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_ids())
def test_yardsticks_stay_below_the_cap(case):
    """Y(case) <= 4000 u: the GPU bound FACTOR * Y never exceeds 3.6e-12 (measured: at most 1774 u, the oracle at
    D = 2049).  A case that breaks this gets a better-conditioned signal, never a looser cap."""
    assert DC.FACTOR == 8.0
    e = DC.evaluated(case)
    print("%s: e1 %.1f u, e2 %.1f u" % (case["id"], e["e1"] / U, e["e2"] / U))
    assert DC.Y_FLOOR <= e["Y"] <= CAP, (case["id"], e["e1"] / U, e["e2"] / U)
    assert e["Y"] == max(DC.Y_FLOOR, e["e1"], e["e2"])


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_ids())
def test_bound_rejects_one_constant_off_by_1e_11(case):
    """For every k, the reference's answer with the caller's constant k times 1 + 1e-11 misses the GPU bound: every
    bound state's soliton lies inside the window, no constant is invisible (measured: at least 3.6 bounds away)."""
    e = DC.evaluated(case)
    for k in range(case["bs"].size):
        err = R.error(DC.reference(case, (k, 1.0 + 1e-11)), e["q_ref"])
        assert err > DC.bound(case), (case["id"], k, err / U, DC.bound(case) / U)


# ---- the ks == 0 record ----------------------------------------------------------------------------------------------
def test_skipped_step_at_ks_zero_is_another_function():
    """Where ks = -|q|^2 - lambda^2 == 0 exactly the reference skips the half step (an identity step); the kernels and
    tests/darboux_ref.py take the limit sinh(k h)/k -> h, which is what the reference's own forward scatterer does.  On
    ks_zero_tails the oracle, which restates the skip, is 0.4 away from the reference -- and within a few u of it once
    the bound state moves off the set of measure zero."""
    c = DC.BY_ID["ks_zero_tails"]
    e = DC.evaluated(c)
    skip = R.error(DC.oracle_double(c, skip_ks_zero=True), e["q_ref"])
    print("oracle with the skip: %.3g (%.3g u); with the limit: %.1f u" % (skip, skip / U, e["e1"] / U))
    assert skip > 1e-3
    assert e["e1"] <= CAP
    bs, nc = R.prepared(c["bs"], c["nc"], False)
    same = R.error(R.cdt_ref(bs, nc, DC.seed_samples(c), c["T"], skip_ks_zero=True), DC.oracle_double(c))
    assert same <= CAP                       # the skip restated in long double is the oracle's function
    off = dict(c, id="ks_zero_tails_off", bs=DC._c(c["bs"] * (1 + 2.0 ** -40)))
    assert R.error(DC.oracle_double(off), DC.reference(off)) <= CAP


# ---- coverage --------------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_discrete_part_is_in_a_case(emu):  # noqa: F811
    inst = set(kernel_list(emu))
    ds = {n for n in inst if n.startswith(DC.DS_PREFIXES)}
    assert ds == {"KInvSolitons", "KInvCdt", "KInvDsPrep"}, sorted(ds)
    eig = set(DC.K_CDT) - {"KInvCdt"}        # the launches of nft_bs_eigenfunctions and the half-step signal
    assert eig <= inst, sorted(eig - inst)
    covered = {k for c in DC.CASES for k in c["kernels"]} | {DC.K_PREP}
    assert covered == ds | eig, (sorted(covered - ds - eig), sorted((ds | eig) - covered))


def test_table_has_the_sizes_and_combinations():
    ids = DC.case_ids()
    assert len(set(ids)) == len(ids)
    for cid in ("K1", "K5_sech", "K12_imag", "K16_wide", "K32_wide", "K3_hugeb", "K2_bigT", "K4_right", "K4_left",
                "ks_zero_tails", "ks_zero_K2", "addsoliton_D64", "addsoliton_D512"):
        assert cid in DC.BY_ID
    assert {c["D"] for c in MODE0} >= {2, 3, 256, 257, 512, 513}
    assert {c["D"] for c in MODE1} >= {2, 3, 9, 10, 64, 300, 2049, 2050}
    assert max(c["D"] for c in DC.CASES) <= 2050
    for mode in (0, 1):
        assert any(c["dstype"] == DC.RESIDUES for c in DC.CASES if c["mode"] == mode)
        assert any(not (c["T"][0] <= 0 <= c["T"][1]) for c in DC.CASES if c["mode"] == mode)
    for c in DC.CASES:
        assert c["T"] == ((-1.0, 1.0) if c["D"] <= 10 else c["T"]) and (c["D"] <= 10 or c["T"][1] - c["T"][0] >= 8)
        assert np.all(c["bs"].imag > 0)
    gap = DC.seed_samples(DC.BY_ID["gap_K4"])
    assert 4 <= np.count_nonzero(gap == 0) < gap.size
    pl, l = DC.seed_samples(DC.BY_ID["ks_zero_tails"]), DC.BY_ID["ks_zero_tails"]["bs"][0]
    assert np.count_nonzero(-np.abs(pl) ** 2 - l * l == 0) > 10
    assert set(DC.BATCH_GROUPS) <= set(ids) and len(DC.EXCLUDED) == 2
    for cid in DC.BATCH_GROUPS:
        sig = DC.batch_signals(DC.BY_ID[cid])
        assert len({s["id"] for s in sig}) == 3
