"""The batched inverse with a discrete spectrum (capi.InversePlan(K=...): fnft_amd_inverse_plan_create_discrete /
fnft_amd_nsev_inverse_discrete_device) on the GPU: every slot against the drop-in fnft_nsev_inverse run on that signal
alone (bitwise for norming constants), the reference's error bounds, independence of the slots with per-signal status,
the host-side call checks, a batch beyond one launch's grid and a realistic size."""

import numpy as np
import pytest

import inverse_cases as IC

pytestmark = pytest.mark.gpu
TAGS = ("2split2A", "2split2_modal")
FNFT_EC_INVALID_ARGUMENT = 2
FNFT_EC_SANITY_CHECK_FAILED = 7


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


def xi_of(capi):
    return lambda D, T, M: capi.nsev_inverse_XI(D, T, M)[1]


def c128(rows):
    return np.ascontiguousarray(np.stack(rows), np.complex128)


def run_batch(capi, torch, D, M, opts, bs_rows, nc_rows, cs_rows=None, XI=None, T=(-1.0, 1.0), seed_rows=None,
              stream=None):
    """One batched call: (rc of finish, q[B, D], status[B], warnings[B]).  The inputs are checked to be unchanged."""
    bs, nc = c128(bs_rows), c128(nc_rows)
    B, K = bs.shape
    plan = capi.InversePlan(D, M, B, opts, K=K)
    try:
        dbs = torch.from_numpy(bs.reshape(-1)).to("cuda")
        dnc = torch.from_numpy(nc.reshape(-1)).to("cuda")
        cs = None if cs_rows is None else c128(cs_rows)
        dcs = None if cs is None else torch.from_numpy(cs.reshape(-1)).to("cuda")
        if seed_rows is None:
            dq = torch.full((B * D,), complex("nan"), dtype=torch.complex128, device="cuda")
        else:
            dq = torch.from_numpy(c128(seed_rows).reshape(-1)).to("cuda")
        sp = 0 if stream is None else stream.cuda_stream
        torch.cuda.synchronize()
        rc = plan.run_device_discrete(0 if dcs is None else dcs.data_ptr(), dbs.data_ptr(), dnc.data_ptr(),
                                      dq.data_ptr(), XI, list(T), 1, sp)
        assert rc == 0, (rc, capi.last_error())
        rcf, st, wn = plan.finish(sp)
        q = dq.cpu().numpy().reshape(B, D)
        assert np.array_equal(dbs.cpu().numpy().reshape(B, K), bs)
        assert np.array_equal(dnc.cpu().numpy().reshape(B, K), nc)
        if cs is not None:
            assert np.array_equal(dcs.cpu().numpy().reshape(cs.shape), cs)
    finally:
        plan.close()
    return rcf, q, st, wn


def drop_in(capi, D, M, opts, bs, nc, cs=None, XI=None, T=(-1.0, 1.0), seed=None):
    # a copy of contspec: the drop-in multiplies the Blaschke factors into it
    return capi.fnft_nsev_inverse(M, None if cs is None else np.array(cs, np.complex128), XI, bs, nc, D, list(T), 1,
                                  opts, q_seed=seed)


def make_case(capi, name, dstype):
    """(case, proper): the inverse_cases case; proper = the case's norming constants / residues match dstype (its
    reference bound applies).  Cases that only give norming constants pass the same values as residues."""
    kind, _, tag = name.partition(":")
    xo = xi_of(capi)
    if kind == "multisoliton":
        return IC.multisoliton_cdt(dstype), True
    if kind == "addsoliton":
        return IC.addsoliton_cdt(512, dstype), True
    if kind == "against_forward":
        case = IC.against_forward_w_discrete(tag, dstype, 512)
        XI = xo(case["D"], case["T"], case["M"])
        rc, bs, nc, res, cs = capi.fnft_nsev_ds(case["q_exact"], case["T"], discretization="2SPLIT4B", M=case["M"],
                                                XI=XI, K=10)
        assert rc == 0 and bs.size == 3
        case.update(contspec=cs[:case["M"]], XI=XI, bound_states=bs,
                    normconsts=nc if dstype == "NORMING_CONSTANTS" else res)
        return case, True
    if kind == "truncated":
        case = IC.truncated_soliton(tag, 512, xo)
    else:
        case = IC.b_cases(kind, True, tag, 0, xo)
    case["opts"] = dict(case["opts"], discspec_type=dstype)
    return case, dstype == "NORMING_CONSTANTS"


def slots(case):
    """Three slots: the case; its bound states (and constants) in reverse order; other constants, bound states moved
    by 0.03 along the real axis, the continuous part and the seed scaled."""
    bs, nc = np.asarray(case["bound_states"], np.complex128), np.asarray(case["normconsts"], np.complex128)
    cs, seed = case.get("contspec"), case.get("q_seed")
    out = [(bs, nc, cs, seed), (bs[::-1].copy(), nc[::-1].copy(), cs, seed),
           (bs + 0.03, nc * (0.9 * np.exp(0.3j)), None if cs is None else 0.8 * np.asarray(cs),
            None if seed is None else 0.9 * np.asarray(seed))]
    return out


def run_slots(capi, torch, case, sl):
    M = case["M"]
    cs_rows = None if M == 0 else [s[2] for s in sl]
    seed_rows = None if case.get("q_seed") is None else [s[3] for s in sl]
    return run_batch(capi, torch, case["D"], M, case["opts"], [s[0] for s in sl], [s[1] for s in sl], cs_rows,
                     case.get("XI"), case["T"], seed_rows)


CASES = (["multisoliton", "addsoliton"] + ["truncated:" + t for t in TAGS] + ["b_of_xi:" + t for t in TAGS]
         + ["B_of_tau:" + t for t in TAGS] + ["against_forward:" + t for t in TAGS])


# ---- 1. every slot against the drop-in, and the reference's bounds -------------------------------------------------
@pytest.mark.parametrize("dstype", ("NORMING_CONSTANTS", "RESIDUES"))
@pytest.mark.parametrize("name", CASES)
def test_every_slot_equals_the_drop_in(capi, torch, name, dstype):
    case, proper = make_case(capi, name, dstype)
    sl = slots(case)
    rc, q, st, wn = run_slots(capi, torch, case, sl)
    assert rc == 0 and (st == 0).all(), (rc, st)
    worst = 0.0
    for b, (bs, nc, cs, seed) in enumerate(sl):
        r0, q0 = drop_in(capi, case["D"], case["M"], case["opts"], bs, nc, cs, case.get("XI"), case["T"], seed)
        assert r0 == 0, capi.last_error()
        # residues become norming constants on the device (KInvDsPrep), the drop-in converts them on the host; the
        # device repeats the host's complex arithmetic operation for operation, so both agree bitwise as well
        worst = max(worst, float(np.max(np.abs(q[b] - q0)) / np.max(np.abs(q0))))
        assert np.array_equal(q[b], q0), (b, worst)
    print("%s %s: max |q_batch - q_drop_in| / max |q| = %.3e" % (name, dstype, worst))
    if proper:
        err = float(np.sum(np.abs(q[0] - case["q_exact"])) / np.sum(np.abs(case["q_exact"])))
        assert err < case["bound"], (err, case["bound"])


# ---- 2. independence of the slots, per-signal status ----------------------------------------------------------------
def eight_slots(capi):
    case = IC.b_cases("b_of_xi", True, "2split2A", 0, xi_of(capi))
    bs0, nc0, cs0 = case["bound_states"], case["normconsts"], np.asarray(case["contspec"])
    rows = []
    for s in range(8):
        bs = bs0 + 0.02 * s
        nc = nc0 * np.exp(0.2j * s) * (1.0 - 0.05 * s)
        rows.append([bs, nc, cs0 * (1.0 - 0.04 * s)])
    rows[2][0] = rows[2][0].copy()
    rows[2][0][1] = 0.5 - 0.2j                 # Im lambda <= 0
    rows[5][0] = rows[5][0].copy()
    rows[5][0][2] = rows[5][0][0]              # a bound state twice
    return case, rows


def test_slots_are_independent(capi, torch):
    case, rows = eight_slots(capi)
    D, M, opts, XI, T = case["D"], case["M"], case["opts"], case["XI"], case["T"]
    rc, q, st, wn = run_batch(capi, torch, D, M, opts, [r[0] for r in rows], [r[1] for r in rows],
                              [r[2] for r in rows], XI, T)
    codes = []
    for b, (bs, nc, cs) in enumerate(rows):
        r0, q0 = drop_in(capi, D, M, opts, bs, nc, cs, XI, T)
        codes.append(r0)
        assert st[b] == r0, (b, st[b], r0)
        if r0 == 0:
            assert np.array_equal(q[b], q0)
    assert codes[2] == FNFT_EC_SANITY_CHECK_FAILED and codes[5] == -FNFT_EC_SANITY_CHECK_FAILED
    assert rc == codes[2]
    for b in (0, 3, 7):
        _, q1, st1, _ = run_batch(capi, torch, D, M, opts, [rows[b][0]], [rows[b][1]], [rows[b][2]], XI, T)
        assert st1[0] == 0 and np.array_equal(q1[0], q[b])
    good = [b for b in range(8) if b not in (2, 5)]
    _, q6, st6, _ = run_batch(capi, torch, D, M, opts, [rows[b][0] for b in good], [rows[b][1] for b in good],
                              [rows[b][2] for b in good], XI, T)
    assert (st6 == 0).all() and np.array_equal(q6, q[good])


# ---- 3. host-side call checks ---------------------------------------------------------------------------------------
def test_host_side_call_checks(capi, torch):
    D, K, B, T = 16, 2, 2, [-1.0, 1.0]
    bs = torch.from_numpy(np.array([1j, 2j, 1j, 2j])).to("cuda")
    nc = torch.ones(B * K, dtype=torch.complex128, device="cuda")
    q = torch.full((B * D,), complex("nan"), dtype=torch.complex128, device="cuda")
    cs = torch.full((B * 2 * D,), 0.01, dtype=torch.complex128, device="cuda")
    XI = capi.nsev_inverse_XI(D, T, 2 * D)[1]
    p = capi.InversePlan(D, 0, B, None, K=K)
    pc = capi.InversePlan(D, 2 * D, B, None, K=K)
    p0 = capi.InversePlan(D, 2 * D, B, None)
    try:
        b, n, qq, c = bs.data_ptr(), nc.data_ptr(), q.data_ptr(), cs.data_ptr()
        assert p.run_device_discrete(0, b, n, qq, None, T, -1) == FNFT_EC_SANITY_CHECK_FAILED
        assert p.run_device_discrete(0, b, n, qq, None, T, 0) == FNFT_EC_INVALID_ARGUMENT
        assert p.run_device_discrete(0, 0, n, qq, None, T, 1) == FNFT_EC_INVALID_ARGUMENT
        assert p.run_device_discrete(0, b, 0, qq, None, T, 1) == FNFT_EC_INVALID_ARGUMENT
        assert p.run_device_discrete(0, b, n, 0, None, T, 1) == FNFT_EC_INVALID_ARGUMENT
        assert p.run_device_discrete(0, b, n, qq, None, [1.0, -1.0], 1) == FNFT_EC_INVALID_ARGUMENT
        assert p.run_device_discrete(c, b, n, qq, None, T, 1) == FNFT_EC_INVALID_ARGUMENT     # contspec with M = 0
        assert pc.run_device_discrete(0, b, n, qq, XI, T, 1) == FNFT_EC_INVALID_ARGUMENT      # no contspec, M > 0
        assert pc.run_device_discrete(c, b, n, qq, None, T, 1) == FNFT_EC_INVALID_ARGUMENT    # no XI
        assert pc.run_device_discrete(c, b, n, qq, XI, T, -1) == FNFT_EC_SANITY_CHECK_FAILED
        # the run call of the other kind of plan
        assert p.run_device(c, qq, XI, T, 1) == -FNFT_EC_INVALID_ARGUMENT
        assert p0.run_device_discrete(c, b, n, qq, XI, T, 1) == -FNFT_EC_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert np.isnan(q.cpu().numpy()).all(), "nothing may have been enqueued"
        # the drop-in's codes for the same calls
        nb = np.array([1j, 2j])
        assert drop_in(capi, D, 0, None, nb, np.ones(2))[0] == 0
        assert capi.fnft_nsev_inverse(0, None, None, nb, np.ones(2), D, T, -1)[0] == FNFT_EC_SANITY_CHECK_FAILED
        assert capi.fnft_nsev_inverse(0, None, None, nb, None, D, T, 1)[0] == FNFT_EC_INVALID_ARGUMENT
        assert p.workspace_bytes() > 0 and pc.workspace_bytes() > p.workspace_bytes()
    finally:
        p.close()
        pc.close()
        p0.close()


# ---- 4. a batch beyond one launch's grid.y --------------------------------------------------------------------------
def test_seed_method_batch_beyond_the_grid_limit(capi, torch):
    D, K, B, T = 16, 3, 22000, [-4.0, 4.0]      # B*K = 66000 > 65536
    rng = np.random.default_rng(3)
    t = IC.tgrid(T, D)
    amp, w = rng.uniform(0.05, 0.3, B), rng.uniform(-1, 1, B)
    seeds = amp[:, None] * IC.sech(t)[None, :] * np.exp(1j * w[:, None] * t[None, :])
    bs = (rng.uniform(-1, 1, (B, K)) + 1j * (np.arange(1, K + 1)[None, :] * 0.6 + rng.uniform(0, 0.2, (B, K))))
    nc = np.exp(1j * rng.uniform(0, 6.28, (B, K)))
    opts = {"contspec_inversion_method": "USE_SEED_POTENTIAL_INSTEAD"}
    rc, q, st, _ = run_batch(capi, torch, D, 0, opts, list(bs), list(nc), T=T, seed_rows=list(seeds))
    assert rc == 0 and (st == 0).all(), (rc, np.count_nonzero(st))
    per_slice = 65535 // K
    for b in (0, 1, per_slice - 1, per_slice, per_slice + 1, B - 1):
        r0, q0 = drop_in(capi, D, 0, opts, bs[b], nc[b], T=T, seed=seeds[b])
        assert r0 == 0, (b, r0)
        assert np.array_equal(q[b], q0), (b, np.max(np.abs(q[b] - q0)), np.isnan(q[b]).sum())


# ---- 5. realistic size ----------------------------------------------------------------------------------------------
def test_b_of_xi_with_discrete_spectrum_d16384_b64(capi, torch):
    case = IC.b_cases("b_of_xi", True, "2split2_modal", 5, xi_of(capi))
    D, M, opts, XI, T = case["D"], case["M"], case["opts"], case["XI"], case["T"]
    assert D == 1 << 14 and len(case["bound_states"]) == 3
    B = 64
    bs0, nc0, cs0 = case["bound_states"], case["normconsts"], np.asarray(case["contspec"])
    rows = [(bs0 + 0.01 * s, nc0 * np.exp(0.1j * s), cs0 * (1.0 - 0.005 * s)) for s in range(B)]
    rc, q, st, _ = run_batch(capi, torch, D, M, opts, [r[0] for r in rows], [r[1] for r in rows],
                             [r[2] for r in rows], XI, T)
    assert rc == 0 and (st == 0).all()
    for b in (0, 17, 40, 63):
        r0, q0 = drop_in(capi, D, M, opts, *rows[b], XI=XI, T=T)
        assert r0 == 0 and np.array_equal(q[b], q0), b
