"""The layer-peeling path tests without a GPU: the long-double reference of tests/peel_ref.py against the samples the
transfer matrices were built from, the cap on the yardsticks that set the GPU bound (tests/peel_cases.py), the proof
that this bound separates a subtly wrong peeling from a right one, and the coverage of the case table -- every
peeling kernel of the library's instantiation list, every branch of NftLayerPeelingDev::peel / prod."""
import numpy as np
import pytest

import peel_cases as PC
import peel_ref as R
from test_emu_kernels import emu, kernel_list  # noqa: F401  (module fixture: builds and loads tests/emu/libfnft_emu.so)

U = R.U
CAP = 2000 * U


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_ids())
def test_reference_recovers_the_constructed_samples(case):
    """The reference applied to the double-precision transfer matrix returns the samples the matrix was built from,
    up to the rounding of tm times the conditioning (measured: at most 784 u, D2048_a10_km_modal)."""
    e = PC.evaluated(case)
    err = R.error(e["q_ref"], e["q_constructed"])
    assert err <= CAP, (case["id"], err / U)


@pytest.mark.parametrize("D,kappa", PC.groups())
def test_yardsticks_stay_below_the_cap(D, kappa):
    """Y(D, kappa) <= 2000 u: the GPU bound FACTOR * Y never exceeds about 1.8e-12 and cannot hide a failure
    (measured: at most 769 u, the recursion at D = 2048, kappa = -1)."""
    assert PC.FACTOR == 8.0
    y = PC.Y(D, kappa)
    assert PC.Y_FLOOR <= y <= CAP, (D, kappa, y / U)


@pytest.mark.parametrize("D", (256, 1024))
@pytest.mark.parametrize("kappa", (1, -1))
@pytest.mark.parametrize("disc", (PC.MODAL, PC.A2))
def test_bound_rejects_a_subtly_wrong_peeling(D, kappa, disc):
    """The double sequential loop with every Q off by 1e-12, and with the sign of kappa wrong in the update of T21
    only, both miss the GPU bound of the case; the unmodified loop meets it."""
    c = PC.BY_ID[PC.case_id(D, "a10", kappa, disc)]
    e = PC.evaluated(c)
    b = PC.bound(c)
    assert e["e_seq"] < b
    for wrong in (dict(q_factor=1.0 + 1e-12), dict(kappa_t21=-kappa)):
        rc, q = R.peel(e["tm"], c["eps_t"], kappa, disc, np.complex128, **wrong)
        # (kappa = -1 with the sign flipped cannot violate 1 + kappa_step |Q|^2 > 0: the check uses the right kappa and
        # |Q| stays far below 1 on these signals)
        assert rc == 0
        err = R.error(q, e["q_ref"])
        assert err > b, (c["id"], wrong, err / U, b / U)


# ---- coverage -------------------------------------------------------------------------------------------------------
def dispatch(D):
    """NftLayerPeelingDev::run_host restated: (kernels, plan products) of a transfer matrix of D samples.  Blocks of up
    to 256 samples go to the leaf; a product of degree 256, 512 or 1024 is one launch of KPeelProduct<2 deg>, any other
    degree goes through a resident plan (KPeelImport, tree, export); step 4 runs only where the caller wants the
    inverse, which is everywhere but at the top."""
    kernels, plans = set(), set()

    def prod(deg, step):
        if deg in (256, 512, 1024):
            kernels.add("KPeelProduct<%d>" % (2 * deg))
        else:
            kernels.add("KPeelImport")
            plans.add("plan%d:step%d" % (deg, step))

    def peel(deg, want_inverse):
        if deg <= 256:
            kernels.add("KPeelLeaf")
            return
        peel(deg // 2, True)
        prod(deg, 2)
        peel(deg // 2, True)
        if want_inverse:
            prod(deg // 2, 4)

    peel(D, False)
    return kernels, plans


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_ids())
def test_case_lists_the_kernels_its_size_reaches(case):
    kernels, plans = dispatch(case["D"])
    assert set(case["kernels"]) == kernels and len(case["kernels"]) == len(kernels)
    assert set(case["paths"]) == plans and len(case["paths"]) == len(plans)


def test_every_peeling_kernel_is_in_a_case(emu):  # noqa: F811
    inst = {n for n in kernel_list(emu) if n.startswith(PC.PEEL_PREFIX)}
    assert inst, "no peeling kernel in the instantiation list"
    covered = {k for c in PC.CASES for k in c["kernels"]}
    assert inst == covered, (sorted(inst - covered), sorted(covered - inst))


def test_table_has_the_sizes_and_combinations():
    """Every kappa, discretization and signal up to D = 1024 (the `steps` signal up to 32), two combinations and two
    signals at 2048 .. 8192, one case at 16384; ids are unique."""
    assert len(PC.BY_ID) == len(PC.CASES) == 10 * 3 * 4 + 5 * 4 + 3 * 4 + 1
    for D in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        got = {(c["signal"], c["kappa"], c["disc"]) for c in PC.CASES if c["D"] == D}
        sig = ("a06", "a10", "rough") + (("steps",) if D <= 32 else ())
        assert got == {(s, k, d) for s in sig for k in (1, -1) for d in (PC.MODAL, PC.A2)}
    for D in (2048, 4096, 8192):
        got = {(c["signal"], c["kappa"], c["disc"]) for c in PC.CASES if c["D"] == D}
        assert got == {(s, k, d) for s in ("a10", "rough") for k, d in ((1, PC.A2), (-1, PC.MODAL))}
    assert [(c["signal"], c["kappa"], c["disc"]) for c in PC.CASES if c["D"] == 16384] == [("a10", -1, PC.A2)]
    for c in PC.CASES:
        Q = PC.step_parameters(c)
        assert np.max(np.abs(Q)) <= 0.7 * (1 + 4 * U) and np.sum(np.abs(Q)) < 3.5, c["id"]
