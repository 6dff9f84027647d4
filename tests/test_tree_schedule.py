"""Product-tree paths without a GPU: the level schedule of every case of tests/tree_cases.py (the emulator in
schedule-only mode: kernel names, nothing executed), coverage of the tree instantiations, and self-tests of the
extended-precision reference tests/tree_ref.py."""
import ctypes as C

import numpy as np
import pytest

import signals as S
import tree_cases as TC
import tree_ref as R
from test_emu_kernels import emu, kernel_list  # noqa: F401  (module fixture: builds and loads tests/emu/libfnft_emu.so)


def schedule(emu, case):
    emu.emu_tree_schedule.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    rc = emu.emu_tree_schedule(*TC.emu_args(case), buf, len(buf))
    assert rc == 0, (case["id"], rc)
    return [n.replace(" ", "") for n in buf.value.decode().split("\n") if n]


@pytest.fixture(scope="module")
def schedules(emu):  # noqa: F811
    return {c["id"]: schedule(emu, c) for c in TC.CASES}


@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_ids())
def test_case_schedule(schedules, case):
    names = schedules[case["id"]]
    missing = [k for k in case["kernels"] if k not in names]
    assert not missing, (missing, names)


@pytest.fixture(scope="module")
def tree_instantiations(emu):  # noqa: F811
    """The tree kernels of the library's instantiation list: what the units compile and the dispatch switches launch."""
    return [n for n in kernel_list(emu) if n.startswith(TC.TREE_PREFIXES)]


def test_tree_instantiation_list(tree_instantiations):
    assert len(tree_instantiations) == 131 == len(set(tree_instantiations))


def test_tree_instantiation_coverage(schedules, tree_instantiations):
    inst = set(tree_instantiations)
    assert len(inst) == len(tree_instantiations)
    assert set(TC.EXCLUDED) <= inst, sorted(set(TC.EXCLUDED) - inst)
    used = set().union(*schedules.values()) & inst
    # every instantiation is launched by some case, or excluded with a reason; an exclusion that a case reaches is stale
    assert used == inst - set(TC.EXCLUDED), (sorted(inst - set(TC.EXCLUDED) - used), sorted(used & set(TC.EXCLUDED)))
    # every tree kernel a case launches is in the list
    extra = {n for s in schedules.values() for n in s if n.startswith(TC.TREE_PREFIXES)} - inst
    assert not extra, sorted(extra)


# ---- self-tests of the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,n", [(1, 1), (1, 2), (2, 5), (3, 7), (5, 9), (1, 64), (4, 33)])
def test_tree_ref_vs_direct(deg, n):
    rng = np.random.default_rng(17 * deg + n)
    p = 0.4 * (rng.standard_normal((4, n * (deg + 1))) + 1j * rng.standard_normal((4, n * (deg + 1))))
    exact = S.tree_direct(p.astype(np.clongdouble), deg, n)
    m = R.points(6)
    assert R.error(exact, 0, R.tree_ref(p, deg, n, m), m) < 1e-18
    # factors p * 2^40: the product is exact * 2^(40 n) through the exponent bookkeeping
    assert R.error(exact, 40 * n, R.tree_ref(p, deg, n, m, 40), m) < 1e-18
    # the ordering convention: P_0 P_1 ..., not the reverse
    if n > 1:
        rev = S.tree_direct(p.reshape(4, n, deg + 1)[:, ::-1].reshape(4, -1).astype(np.clongdouble), deg, n)
        assert R.error(rev, 0, R.tree_ref(p, deg, n, m), m) > 1e-3


def test_tree_ref_vs_oracle(oracle):
    """The oracle's full products (fmult2x2, akns_fscatter from its own per-sample factors, kdv_fscatter) agree with the
    reference within the exact-factor bound."""
    m = R.points(8)
    c = TC.CASES[TC.case_ids().index("fmult_d2_n300_up40")]
    p = TC.fmult_factors(c)
    d, res, W = oracle.poly_fmult2x2(2, 300, p)
    e = R.error(res, W, R.tree_ref(p, 2, 300, m), m)
    assert e < R.err_bound(TC.BOUND_GENERAL, 1024, 300), e
    q, r, T = TC.akns_signal(dict(n=3000))
    eps_t = (T[1] - T[0]) / (q.size - 1)
    rc, deg0, f = oracle.akns_coeffs(q, r, eps_t, "2SPLIT4B")
    rc2, dd, res, W = oracle.akns_fscatter(q, r, eps_t, "2SPLIT4B")
    assert rc == 0 and rc2 == 0 and dd == deg0 * q.size
    e = R.error(res, W, R.tree_ref(f, deg0, q.size, m), m)
    assert e < R.err_bound(TC.BOUND_SAMPLES, 2 * dd, q.size), e
    u, T = TC.kdv_signal(dict(n=2000))
    eps_t = (T[1] - T[0]) / (u.size - 1)
    rc, deg0, f = oracle.akns_coeffs(u, -np.ones_like(u), eps_t, "2SPLIT3A")
    rc2, dd, res, W = oracle.kdv_fscatter(u, eps_t, "2SPLIT3A", normalize=True)
    assert rc == 0 and rc2 == 0 and dd == deg0 * u.size
    e = R.error(res, W, R.tree_ref(f, deg0, u.size, m), m)
    assert e < R.err_bound(TC.BOUND_REAL, 2 * dd, u.size), e


@pytest.mark.parametrize("deg", [4096, 65536])
def test_metric_sensitivity(oracle, deg):
    """A correct product (the oracle's FFT product of two factors with decaying coefficients) whose coefficients carry
    a systematic relative error of 1e-12 exceeds the bound of exact factors: a uniform error c -> c (1 + 1e-12), and an
    error of 1e-12 max|c| with a phase that turns with j (what a drifting twiddle leaves in every coefficient of an
    inverse transform).  The metric has teeth on products of few long factors; on trees of many factors the n term of
    the bound is larger than such an error (see tree_ref.err_bound)."""
    rng = np.random.default_rng(deg)
    decay = 0.9 ** np.arange(deg + 1)
    p = np.concatenate([decay * (rng.standard_normal((4, deg + 1)) + 1j * rng.standard_normal((4, deg + 1)))
                        for _ in range(2)], axis=1)
    d, res, W = oracle.poly_fmult2x2(deg, 2, p)
    m = R.points(4)
    ref = R.tree_ref(p, deg, 2, m)
    bound = R.err_bound(TC.BOUND_GENERAL, 4 * deg, 2)
    e0 = R.error(res, W, ref, m)
    assert e0 < bound, e0
    drift = 1e-12 * np.max(np.abs(res)) * np.exp(2j * np.pi * 0.37 * np.arange(d + 1))
    for bad in (res * (1 + 1e-12), res + drift):
        e = R.error(bad, W, ref, m)
        assert e > bound and e > 10 * e0, (e, bound, e0)
