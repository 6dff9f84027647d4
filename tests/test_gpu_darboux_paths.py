"""The discrete part of fnft_nsev_inverse on the GPU (KInvSolitons, KInvCdt on the eigenfunctions of
nft_bs_eigenfunctions -- KInvOp in mode INV_DOUBLE_Q, KBsChunk, KBsCombine, KBsPhi, KBsPsi --, KInvDsPrep, the drivers
NftInverseDev::add_discrete and NftInverseDiscBatch::run) against the long-double reference of tests/darboux_ref.py, on
every case of tests/darboux_cases.py.

The bound of a case is not taken from the GPU's own result: it is FACTOR = 8 times Y(case), the larger of two
double-precision CPU yardsticks measured against the same reference on the same inputs (tests/test_darboux_cases_cpu.py
caps Y at 4000 u and shows that 8 Y rejects a result with one norming constant off by 1e-11).

Every case runs through the host-pointer path: the drop-in fnft_nsev_inverse where D is a power of two -- the only sizes
the public entry accepts, as in the reference --, and for the other sizes the driver the drop-in calls after its checks
(fnft_amd__inverse_add_discrete: the same host code and kernels without the size check).  The batched plan runs three
different signals of every power-of-two (D, K) group, each against its own reference."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import darboux_cases as DC
import darboux_ref as R

pytestmark = pytest.mark.gpu

U = R.U
_measured = {}


@pytest.fixture(scope="module")
def capi(lib):
    from fnft_amd import build
    from fnft_amd import capi as c
    assert lib.fnft_amd_device_count() >= 1, c.last_error()
    c.silence_errors()
    lib.fnft_amd__inverse_add_discrete.restype = C.c_int32
    lib.fnft_amd__inverse_add_discrete.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_int, C.c_int]
    yield c
    out = os.environ.get("FNFT_DARBOUX_ERR_JSON")   # optional record of the measured errors (profiles/darboux_errors.json)
    if out:
        ratios = {}
        for m in _measured.values():
            key = "mode%d:D%d" % (m["mode"], m["D"])
            ratios[key] = max(ratios.get(key, 0.0), m["ratio"])
        head = dict(build_id=build.build_id(), unit="u = 2^-53", factor=DC.FACTOR, largest_ratio_per_mode_and_D=ratios)
        with open(out, "w") as f:      # one line per case
            f.write("{\n" + "".join(' %s: %s,\n' % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
            f.write(' "cases": {\n' + ",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in _measured.items()))
            f.write("\n }\n}\n")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def _opts(c):
    o = dict(discspec_type=c["dstype"])
    if c["mode"]:
        o["contspec_inversion_method"] = "USE_SEED_POTENTIAL_INSTEAD"
    return o


def _host_call(capi, lib, c):
    """(rc, q) of the case through the host-pointer path."""
    D, T = c["D"], list(c["T"])
    seed = DC.seed_samples(c) if c["mode"] else None
    if DC.power_of_two(c):
        return capi.fnft_nsev_inverse(0, None, None, c["bs"], c["nc"], D, T, 1, _opts(c), q_seed=seed)
    bs, nc = np.array(c["bs"], np.complex128), np.array(c["nc"], np.complex128)
    q = np.full(D, np.nan + 0j) if seed is None else np.array(seed, np.complex128)
    Tn = np.array(T, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    rc = lib.fnft_amd__inverse_add_discrete(bs.size, vp(bs), vp(nc), D, vp(q), vp(Tn), 0,
                                            1 if c["dstype"] == DC.RESIDUES else 0, 1 if c["mode"] else 0)
    assert np.array_equal(bs, c["bs"]) and np.array_equal(nc, c["nc"])
    return int(rc), q


def _check(c, q, key=None):
    """q within the case's bound of the reference; the figures are printed and recorded before the assertion."""
    e = DC.evaluated(c)
    err, y, b = R.error(q, e["q_ref"]), e["Y"], DC.bound(c)
    _measured[key or c["id"]] = dict(mode=c["mode"], D=c["D"], K=int(c["bs"].size), e_gpu=round(err / U, 2),
                                     e1=round(e["e1"] / U, 2), e2=round(e["e2"] / U, 2), Y=round(y / U, 2),
                                     ratio=round(err / y, 3))
    print("%s: e_gpu %.1f u, e1 %.1f u, e2 %.1f u, Y %.1f u, ratio %.2f" % (key or c["id"], err / U, e["e1"] / U,
                                                                           e["e2"] / U, y / U, err / y))
    assert np.all(np.isfinite(q)) and err < b, (key or c["id"], err / U, b / U)


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_ids())
def test_darboux_path(capi, lib, case):
    rc, q = _host_call(capi, lib, case)
    assert rc == 0, (case["id"], rc, capi.last_error())
    _check(case, q)


_GROUPS = [cid for cid in DC.BATCH_GROUPS if DC.power_of_two(DC.BY_ID[cid])]


@pytest.mark.parametrize("cid", _GROUPS)
def test_batch_of_three(capi, torch, cid):
    """capi.InversePlan(D, 0, 3, opts, K=K).run_device_discrete on three different signals of the group: every slot
    within its own bound (the strides of NftInverseDiscBatch), status 0, the caller's arrays unchanged."""
    sig = DC.batch_signals(DC.BY_ID[cid])
    c0 = sig[0]
    D, K, B = c0["D"], c0["bs"].size, len(sig)
    bs = np.ascontiguousarray(np.stack([c["bs"] for c in sig]), np.complex128)
    nc = np.ascontiguousarray(np.stack([c["nc"] for c in sig]), np.complex128)
    plan = capi.InversePlan(D, 0, B, _opts(c0), K=K)
    try:
        dbs = torch.from_numpy(bs.reshape(-1)).to("cuda")
        dnc = torch.from_numpy(nc.reshape(-1)).to("cuda")
        if c0["mode"]:
            seeds = np.ascontiguousarray(np.stack([DC.seed_samples(c) for c in sig]), np.complex128)
            dq = torch.from_numpy(seeds.reshape(-1)).to("cuda")
        else:
            dq = torch.full((B * D,), complex("nan"), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        rc = plan.run_device_discrete(0, dbs.data_ptr(), dnc.data_ptr(), dq.data_ptr(), None, list(c0["T"]), 1, 0)
        assert rc == 0, (rc, capi.last_error())
        rcf, st, _ = plan.finish(0)
        q = dq.cpu().numpy().reshape(B, D)
        assert np.array_equal(dbs.cpu().numpy().reshape(B, K), bs) and np.array_equal(dnc.cpu().numpy().reshape(B, K), nc)
    finally:
        plan.close()
    assert rcf == 0 and not st.any(), (rcf, st, capi.last_error())
    for s, c in enumerate(sig):
        _check(c, q[s], "batch[%d]%s" % (s, c["id"]))
