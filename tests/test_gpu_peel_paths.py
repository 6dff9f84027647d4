"""Layer peeling on the GPU (NftLayerPeelingDev behind fnft__nse_finvscatter: KPeelLeaf, KPeelProduct<512|1024|2048>,
KPeelImport, the n = 2 product trees and the strided export) against the long-double reference of tests/peel_ref.py,
on every case of tests/peel_cases.py.

The bound of a case is not taken from the GPU's own result: it is FACTOR = 8 times Y(D, kappa), the larger of two
double-precision CPU yardsticks -- the reference's recursion with FFT products (oracle.oracle.nse_finvscatter) and the
plain sequential loop in complex128 -- measured against the same reference on the same transfer matrices
(tests/test_peel_cases_cpu.py caps Y at 2000 u and shows that 8 Y rejects a peeling that is wrong by 1e-12).  Beyond
accuracy: invariance under scaling of the transfer matrix, the resident state of the host-pointer entry over calls of
changing size, sign and discretization, and a call that fails."""
import json
import os

import numpy as np
import pytest

import peel_cases as PC
import peel_ref as R

pytestmark = pytest.mark.gpu

U = R.U
_measured = {}


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import build
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    c.silence_errors()
    yield c
    out = os.environ.get("FNFT_PEEL_ERR_JSON")   # optional record of the measured errors (profiles/peel_errors.json)
    if out:
        ratios = {}
        for k, m in _measured.items():
            if "ratio" in m:
                ratios[str(m["D"])] = max(ratios.get(str(m["D"]), 0.0), m["ratio"])
        head = dict(build_id=build.build_id(), unit="u = 2^-53", factor=PC.FACTOR, largest_ratio_per_D=ratios)
        with open(out, "w") as f:      # one line per case
            f.write("{\n" + "".join(' %s: %s,\n' % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
            f.write(' "cases": {\n' + ",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in _measured.items()))
            f.write("\n }\n}\n")


def _run(capi, c, tm=None):
    rc, q = capi.nse_finvscatter(PC.evaluated(c)["tm"] if tm is None else tm, c["eps_t"], c["kappa"], c["disc"])
    assert rc == 0, (c["id"], rc, capi.last_error())
    return q


def _check(c, q, key=None, **extra):
    """q within the case's bound of the reference; the figures are printed and recorded before the assertion."""
    e = PC.evaluated(c)
    err, y, b = R.error(q, e["q_ref"]), PC.Y(c["D"], c["kappa"]), PC.bound(c)
    _measured[key or c["id"]] = dict(D=c["D"], kappa=c["kappa"], e_gpu=round(err / U, 2), e_seq=round(e["e_seq"] / U, 2),
                                     e_rec=round(e["e_rec"] / U, 2), Y=round(y / U, 2), ratio=round(err / y, 3), **extra)
    print("%s: e_gpu %.1f u, seq %.1f u, rec %.1f u, Y %.1f u, ratio %.2f" % (key or c["id"], err / U, e["e_seq"] / U,
                                                                             e["e_rec"] / U, y / U, err / y))
    assert np.all(np.isfinite(q)) and err < b, (key or c["id"], err / U, b / U)


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_ids())
def test_peel_path(capi, case):
    _check(case, _run(capi, case))


@pytest.mark.parametrize("D", (256, 1024, 4096))
def test_scaled_transfer_matrix(capi, D):
    """tm times 2^100 and 2^-100: peeling only sees ratios, so the reference samples and the bound are those of the
    unscaled case (whether the samples are bitwise those of the unscaled call is recorded, not required)."""
    for c in (c for c in PC.CASES if c["D"] == D and c["signal"] == "a10"):
        tm = PC.evaluated(c)["tm"]
        q0 = _run(capi, c)
        for p in (100, -100):
            q = _run(capi, c, tm * 2.0 ** p)
            _check(c, q, "%s*2^%d" % (c["id"], p), bitwise_equal_to_unscaled=bool(np.array_equal(q, q0)))


def test_resident_state_over_changing_calls(capi):
    """The resident peeler keeps its work arrays (the upper half of T2i zeroed once, depth 0 the largest size so far)
    and one plan per degree from call to call: sizes, signs and discretizations in changing order, and a release in
    between, give every case its bound and every repeated case the bits of its first call (no floating-point atomics
    in these kernels)."""
    big = PC.BY_ID[PC.case_id(8192, "a10", 1, PC.A2)]
    c512 = PC.BY_ID[PC.case_id(512, "a10", -1, PC.MODAL)]
    c2048 = PC.make_case(2048, "a10", 1, PC.MODAL)        # not in the table: its bound is that of the group (2048, +1)
    c256 = PC.BY_ID[PC.case_id(256, "a10", 1, PC.A2)]
    first = {}
    for i, c in enumerate((big, c512, c2048, c256, big, None, c2048)):
        if c is None:
            capi.release_cached(-1)
            continue
        q = _run(capi, c)
        same = np.array_equal(q, first.setdefault(c["id"], q))
        _check(c, q, "resident[%d]%s" % (i, c["id"]), bitwise_equal_to_first_call=bool(same))
        assert same, (i, c["id"])


def test_failed_call_and_the_call_after(capi):
    """kappa = -1 and one reconstructed sample with |Q| = 1.05 at D = 1024: FNFT_EC_OTHER (status bit 4 of the leaf,
    read by run_host), after which the entry releases the resident state; the next calls are within their bounds."""
    tm, eps_t = PC.failing_transfer_matrix(1024)
    assert np.all(np.isfinite(tm))
    assert R.peel_steps(tm, -1)[0] == 5
    rc, _ = capi.nse_finvscatter(tm, eps_t, -1, PC.MODAL)
    assert rc == 5, (rc, capi.last_error())
    for disc in (PC.MODAL, PC.A2):
        c = PC.BY_ID[PC.case_id(1024, "a06", -1, disc)]
        _check(c, _run(capi, c), "after_failure:" + c["id"])
