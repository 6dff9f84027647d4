"""Chirp z-transform paths without a GPU: the launch schedule of every case of tests/chirp_cases.py (the emulator in
schedule-only mode: kernel names from the product's own host code, nothing executed), coverage of the chirp
instantiations, self-tests of the extended-precision reference tests/chirp_ref.py, and the metric's sensitivity."""
import ctypes as C
import re

import numpy as np
import pytest

import chirp_cases as CC
import chirp_ref as R
from test_emu_kernels import emu, kernel_list  # noqa: F401  (module fixture: builds and loads tests/emu/libfnft_emu.so)

CLD = np.clongdouble


def schedule(emu, case):
    emu.emu_chirp_schedule.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                       C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    rc = emu.emu_chirp_schedule(*CC.emu_args(case), buf, len(buf))
    assert rc == 0, (case["id"], rc)
    return [n.replace(" ", "") for n in buf.value.decode().split("\n") if n]


@pytest.fixture(scope="module")
def schedules(emu):  # noqa: F811
    return {c["id"]: schedule(emu, c) for c in CC.CASES}


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_ids())
def test_case_schedule(schedules, case):
    names = schedules[case["id"]]
    missing = [k for k in CC.kernels(case) if k not in names]
    assert not missing, (missing, names)
    # the chirp runs at exactly the case's column length (the length is the product's choice, not re-derived here)
    n1 = {int(m) for n in names for m in re.findall(r"^KChirpCol(?:Fwd|Inv)<(\d+),", n)}
    if case["entry"] != "resample":
        assert n1 == {case["N1"]}, (n1, names)
    unwanted = [k for k in case["absent"] if k in names]
    assert not unwanted, (unwanted, names)


@pytest.fixture(scope="module")
def chirp_instantiations(emu):  # noqa: F811
    """The chirp kernels of the library's instantiation list: what the units compile and the dispatch switches launch."""
    return [n for n in kernel_list(emu) if n.startswith("KChirp")]


def test_chirp_instantiation_list(chirp_instantiations):
    assert len(chirp_instantiations) == 66 == len(set(chirp_instantiations))


def test_chirp_instantiation_coverage(schedules, chirp_instantiations):
    inst = set(chirp_instantiations)
    assert set(CC.EXCLUDED) <= inst, sorted(set(CC.EXCLUDED) - inst)
    used = set().union(*schedules.values()) & inst
    # every instantiation is launched by some case, or excluded with a reason; an exclusion that a case reaches is stale
    assert used == inst - set(CC.EXCLUDED), (sorted(inst - set(CC.EXCLUDED) - used), sorted(used & set(CC.EXCLUDED)))
    extra = {n for s in schedules.values() for n in s if n.startswith("KChirp")} - inst
    assert not extra, sorted(extra)


# ---- self-tests of the reference ------------------------------------------------------------------------------------
def _direct(p, A, W, m):
    """sum_n p[deg-n] A^-n W^(n m) term by term in clongdouble from long-double logs (powers by exp, no recurrence)."""
    la, lw = R.ld_log(A), R.ld_log(W)
    deg = p.size - 1
    out = []
    for mm in m:
        s = CLD(0)
        for n in range(deg + 1):
            e = (-n * la[0] + n * int(mm) * lw[0]) + 1j * (-n * la[1] + n * int(mm) * lw[1])
            s += CLD(p[deg - n]) * np.exp(CLD(e))
        out.append(s)
    return np.array(out, CLD)


@pytest.mark.parametrize("deg,A,W", [(40, 1.01 * np.exp(0.3j), np.exp(-0.2j)),           # W below the axis, |A| > 1
                                     (33, 0.97 * np.exp(-0.1j), 1.001 * np.exp(0.05j)),  # |A| < 1, |W| != 1
                                     (0, 1.0, np.exp(0.7j))])
def test_chirpz_ref_vs_direct(deg, A, W):
    rng = np.random.default_rng(deg)
    p = rng.standard_normal(deg + 1) + 1j * rng.standard_normal(deg + 1)
    m = np.array([0, 3, 17, 50, 123])
    v, mass = R.chirpz_ref(p, A, W, m)
    assert R.error(v, _direct(p, A, W, m), mass) < 1e-18
    # mass = sum |c_n| |A|^-n
    n = np.arange(deg + 1)
    assert abs(float(mass) - np.sum(np.abs(p[::-1]) * np.abs(A) ** -n)) < 1e-12 * float(mass)


@pytest.mark.parametrize("ln,sign", [(37, -1), (64, +1), (1000, -1)])
def test_dft_ref_residues(ln, sign):
    """DFT mode: powers from the exact residue (n m) mod len, against a long-double DFT of the same length."""
    rng = np.random.default_rng(ln)
    x = rng.standard_normal(ln) + 1j * rng.standard_normal(ln)
    m = np.arange(ln)
    v, mass = R.chirpz_ref(x, 1.0, 1.0, m, dft=(ln, sign))
    ang = sign * 2 * R._PI * ((np.outer(m, np.arange(ln)) % ln).astype(np.longdouble) / np.longdouble(ln))
    ref = (np.cos(ang) + 1j * np.sin(ang)).astype(CLD) @ x.astype(CLD)
    assert R.error(v, ref, mass) < 1e-18
    np.testing.assert_allclose(v.astype(np.complex128), np.fft.fft(x) if sign < 0 else np.fft.ifft(x) * ln,
                               rtol=0, atol=1e-12 * float(mass))


@pytest.mark.parametrize("D,x", [(64, 0.29), (63, 0.29), (17, -1.7), (40, 3.0), (5, 0.5)])
def test_resample_ref_vs_explicit(D, x):
    """The closed-form resampler against an explicit long-double DFT -> phase ramp -> inverse DFT (D <= 64),
    the phi -> 0 limit (integer shift x) included."""
    rng = np.random.default_rng(D)
    q = rng.standard_normal(D) + 1j * rng.standard_normal(D)
    eps_t = 0.125      # delta = x eps_t exactly: x = 3 is an integer shift
    delta = x * eps_t
    k = np.arange(D)
    f = np.where(k < D // 2, k, k - D).astype(np.longdouble)
    ang = -2 * R._PI * (np.outer(k, k) % D).astype(np.longdouble) / np.longdouble(D)
    F = (np.cos(ang) + 1j * np.sin(ang)).astype(CLD)
    ramp = 2 * R._PI * (np.longdouble(delta) / (np.longdouble(D) * np.longdouble(eps_t))) * f
    X = (F @ q.astype(CLD)) * (np.cos(ramp) + 1j * np.sin(ramp)).astype(CLD)
    ref = np.conj(F) @ X / np.longdouble(D)
    got = R.resample_ref(q, eps_t, delta, k)
    assert float(np.max(np.abs(got - ref))) < 1e-17 * float(np.sum(np.abs(q)))


def test_chirp_ref_vs_oracle(oracle):
    """The oracle's (double-precision) poly_chirpz and misc_resample agree with the reference within the bounds."""
    c = CC.CASES[CC.case_ids().index("chirpz_N2_tight_fit")]
    p, A, W, m0 = CC.chirpz_inputs(c)
    L = CC.ROW * c["N1"]
    m = CC.out_points(c, c["M"], [m0])
    ref, mass = R.chirpz_ref(p, A, W, m)
    x = oracle.poly_chirpz(p, A, W, c["M"])
    e = R.error(x[m], ref, mass)
    assert e < R.err_bound(CC.BOUND_RAW, L, R.phi(L, A, W)), e
    c = CC.CASES[CC.case_ids().index("resample_N2_D4093")]
    q, eps_t, delta = CC.resample_inputs(c)
    rc, qn = oracle.misc_resample(q, eps_t, delta)
    assert rc == 0
    j = CC.out_points(c, q.size)
    e = float(np.max(np.abs(qn[j] - R.resample_ref(q, eps_t, delta, j)))) / R.resample_mass(q)
    assert e < R.err_bound(CC.BOUND_DFT, CC.ROW * c["N1"]), e


def _perturbed(x, idx):
    """The two systematic errors of 1e-12 the metric must see: uniform relative, and 1e-12 max|x| with a phase that
    turns with the output index (a drifting twiddle)."""
    drift = 1e-12 * np.max(np.abs(x)) * np.exp(2j * np.pi * 0.37 * np.asarray(idx))
    return x * (1 + 1e-12), x + drift


def test_metric_sensitivity_raw(oracle):
    c = CC.CASES[CC.case_ids().index("chirpz_N4_M7_ring_out")]
    p, A, W, m0 = CC.chirpz_inputs(c)
    L = CC.ROW * c["N1"]
    m = CC.out_points(c, c["M"], [m0])
    ref, mass = R.chirpz_ref(p, A, W, m)
    x = oracle.poly_chirpz(p, A, W, c["M"])[m]
    bound = R.err_bound(CC.BOUND_RAW, L, R.phi(L, A, W))
    e0 = R.error(x, ref, mass)
    assert e0 < bound, e0
    for bad in _perturbed(x, m):
        e = R.error(bad, ref, mass)
        assert e > bound and e > 10 * e0, (e, bound, e0)


def test_metric_sensitivity_dft(oracle):
    c = CC.CASES[CC.case_ids().index("resample_N4_D8191")]
    q, eps_t, delta = CC.resample_inputs(c)
    rc, qn = oracle.misc_resample(q, eps_t, delta)
    assert rc == 0
    j = CC.out_points(c, q.size)
    ref = R.resample_ref(q, eps_t, delta, j)
    mass = R.resample_mass(q)
    bound = R.err_bound(CC.BOUND_DFT, CC.ROW * c["N1"])
    e0 = R.error(qn[j], ref, mass)
    assert e0 < bound, e0
    for bad in _perturbed(qn[j], j):
        e = R.error(bad, ref, mass)
        assert e > bound and e > 10 * e0, (e, bound, e0)


def test_metric_sensitivity_epilogue(oracle):
    """rho of the NSE epilogue from the oracle's chirp values of a transfer matrix (first-order quotient metric)."""
    c = CC.CASES[CC.case_ids().index("tm_MODAL_both_N2_W7")]
    tm = CC.tm_inputs(c)[0]
    T, XI = CC.grid(c)
    M, D = c["M"], c["D"]
    L = CC.ROW * c["N1"]
    m = CC.out_points(c, M)
    ref = R.nsev_epilogue_ref(tm, 0, T, XI, M, D, 1, True, m)
    A, V = R.nsev_grid(T, XI, M, D, 1)
    H11 = oracle.poly_chirpz(tm[0], A, V, M)[m]
    H21 = oracle.poly_chirpz(tm[2], A, V, M)[m]
    xi, pf_rho, _, _ = R.nsev_phase_factors(T, XI, M, D, 1, True, m)
    rho = (H21 / H11) * np.exp(1j * (xi * pf_rho).astype(np.float64))
    bound = R.err_bound(CC.BOUND_NSE, L, R.phi(L, A, V) + ref["phi_pf"])
    e0 = R.quotient_error(rho, ref["rho"], ref["H11"], ref["mass"])
    assert e0 < bound, e0
    for bad in _perturbed(rho, m):
        e = R.quotient_error(bad, ref["rho"], ref["H11"], ref["mass"])
        assert e > bound and e > 10 * e0, (e, bound, e0)
