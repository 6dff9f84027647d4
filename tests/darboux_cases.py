"""Case table and yardsticks of the Darboux path tests (tests/test_darboux_cases_cpu.py, tests/test_darboux_emu.py,
tests/test_gpu_darboux_paths.py): the discrete part of fnft_nsev_inverse -- KInvSolitons, KInvCdt on the eigenfunctions
of nft_bs_eigenfunctions, KInvDsPrep, NftInverseDev::add_discrete and NftInverseDiscBatch::run -- against the
long-double reference of tests/darboux_ref.py.

A case is a dict: id, mode (0 pure solitons, 1 Darboux steps on a seed), D, T, bs and nc (bound states and norming
constants or residues, as the caller passes them: unsorted where the case says so), dstype, seed (a name, see
seed_samples; None in mode 0) and kernels (the launches of NftInverseDiscBatch::run after check_and_sort, in order).

Sizes.  KInvSolitons and KInvCdt take one sample per lane in workgroups of 256: D = 2, 3, 256, 257, 512, 513.  The
eigenfunctions run on the half-step signal of D2 = 2 (D - 1) samples in chunks of nft_bs_chunk_len = 16, and
KBsCombine gives each of its 256 lanes ceil(nchunk / 256) chunks: D = 2, 3 (one partial chunk), 9 (exactly one chunk),
10 (two chunks, the last of 2 samples), 64, 300, 2048 (256 chunks, the last of 14), 2049 (256 full chunks), 2050 (257
chunks: the first size at which a lane owns two).  T = [-1, 1] for D <= 10 (on [-12, 12] two or three samples say
nothing: the double oracle itself is then off by 5e3 to 2.6e5 u), [-12, 12] or wider from D = 64 on.

The public entries accept powers of two only (fnft_nsev_inverse and fnft_amd_inverse_plan_create_discrete return
FNFT_EC_INVALID_ARGUMENT otherwise, as the reference does).  On the GPU the other sizes go through the host-pointer
driver behind the drop-in (fnft_amd__inverse_add_discrete, no size check: the same NftInverseDev::add_discrete and the
same kernels), and the batched plan runs the power-of-two groups; in the emulator NftInverseDiscBatch runs every size.

The GPU's (and the emulator's) error may be FACTOR times Y(case) = max(4 u, e1, e2), the errors of two double-precision
CPU runs against the same reference on the same inputs -- see evaluated().  What differs legitimately between numpy and
the kernels (FMA contraction, the device's exp and sincos, Smith's division, the chunked association) changes the error
by small constants, not its growth.  FACTOR is the value of the layer-peeling tests and is not raised on the evidence of
the GPU's own error.  Largest measured e_gpu / Y per mode and D on an MI355X (profiles/darboux_errors.json, batched
calls included; DESIGN.md section 2, "Darboux stage against a long-double reference"):
  mode 0   D      2     3     64    200   256   257   512   513   1001
           ratio  0.33  0.58  0.55  0.71  0.73  1.01  0.32  0.71  0.006
  mode 1   D      2     3     9     10    64    128   300   512   2048  2049  2050
           ratio  0.89  1.13  1.04  0.70  1.36  0.93  0.68  0.61  0.97  0.55  0.42
Tried against this bound in the emulator with deliberately wrong copies of the kernels: the recursion's f or the Darboux
step's S2 off by 1e-10 fails every case of its mode (ratios 6e2 .. 5e5), the half-step signal as q'[i] = q[i/2] every
mode-1 case with a seed (1e10 .. 8e14), the per-signal stride of the chunk boundary vectors one chunk short the mode-1
batches from D = 10 on (2e6 .. 4e14), the reference's skipped step at ks == 0 the two ks_zero cases (7e13 .. 1e14).
"""
import numpy as np

import darboux_ref as R
import inverse_cases as IC

U = R.U
FACTOR = 8.0
Y_FLOOR = 4 * U
NORMCONSTS, RESIDUES = "NORMING_CONSTANTS", "RESIDUES"

K_SOLITONS = ["KInvSolitons"]
K_CDT = ["KInvOp", "KBsChunk<false>", "KBsCombine<false>", "KBsPhi", "KBsChunk<true>", "KBsCombine<true>", "KBsPsi",
         "KInvCdt"]
K_PREP = "KInvDsPrep"            # check_and_sort, in front of either list
DS_PREFIXES = ("KInvSolitons", "KInvCdt", "KInvDsPrep")

EXCLUDED = {
    "chunk lengths above 16": "nft_bs_chunk_len exceeds 16 only for D2 > 16 * 16384, that is D > 131073: the "
                              "reference's Python loop over the half steps alone would take minutes",
    "RESIDUES on top of a continuous part": "a(lambda_k) of the seed through nft_bs_forward on D samples (stage 1 of "
                                            "KInvDsPrep) belongs with the tests of the bound-state scatterer",
}

K4_BS = np.array([0.5 + 1.1j, -0.7 + 0.8j, 0.1 + 0.5j, 1.3 + 0.3j])
K4_NC = np.array([1.5, -0.7j, 2 + 1j, -0.2])
K8_BS = np.concatenate([K4_BS, [-1.2 + 0.9j, 0.6 + 1.4j, -0.3 + 0.35j, 0.9 + 0.65j]])
K8_NC = np.concatenate([K4_NC, [0.8j, -1.2, 0.5 - 0.5j, 3.0]])
SIDE_BS = np.array([1 + 1.2j, -0.5 + 0.9j, 0.2 + 0.6j, 0.4j])
_SIDE_ETA, _SIDE_POS, _SIDE_ARG = SIDE_BS.imag, np.array([3.0, 5.0, 6.0, 4.0]), np.array([0.3, np.pi, np.pi / 2, 0.0])


def _c(a):
    a = np.array(a, np.complex128)
    a.setflags(write=False)
    return a


def _case(cid, mode, D, T, bs, nc, dstype=NORMCONSTS, seed=None):
    assert (seed is None) == (mode == 0)
    return dict(id=cid, mode=mode, D=D, T=(float(T[0]), float(T[1])), bs=_c(bs), nc=_c(nc), dstype=dstype, seed=seed,
                kernels=list(K_CDT if mode else K_SOLITONS))


def _table():
    k = np.arange(12)
    k16, k32 = np.arange(16), np.arange(32)
    sech5 = IC.multisoliton_cdt(NORMCONSTS, 256)
    add = {D: IC.addsoliton_cdt(D, NORMCONSTS) for D in (64, 512)}
    m0 = [
        _case("K1", 0, 256, (-12, 12), [0.3 + 0.8j], [1.7 * np.exp(0.4j)]),
        _case("K5_sech", 0, 256, sech5["T"], sech5["bound_states"], sech5["normconsts"]),
        _case("K12_imag", 0, 256, (-20, 20), 1j * (0.4 + 0.35 * k), (-1.0) ** k),
        # equal imaginary parts and ascending runs: the exchange sort moves every entry
        _case("K16_wide", 0, 512, (-24, 24), 0.5 * k16 - 3.75 + 1j * (0.8 + 0.4 * (k16 % 3)), np.exp(2j * k16)),
        _case("K32_wide", 0, 512, (-30, 30), 0.4 * k32 - 6.2 + 1j * (0.7 + 0.3 * (k32 % 4)),
              np.exp(0.7j * k32) * 2.0 ** ((k32 % 7) - 3)),
        # solitons at t = ln|b| / (2 Im lambda) = 34.5, -28.8, 27.6; D odd and T symmetric: t = 0 is sample 128
        _case("K3_hugeb", 0, 257, (-40, 40), [0.5 + 1.0j, -0.3 + 1.2j, 0.2 + 0.5j], [1e30, 1e-30j, -1e12]),
        # exp(+-2 Im lambda t) under- and overflows on both sides; the phase 2 Re lambda t reaches 400; t = 0 is sample 500
        _case("K2_bigT", 0, 1001, (-400, 400), [2j, 0.5 + 1j], [1.0, -1.0]),
        # no sample left of the zero crossing (zc = 0) / none right of it ("no t >= 0": zc = 0 again); the solitons sit
        # at |t| = 3, 5, 6, 4
        _case("K4_right", 0, 200, (1, 9), SIDE_BS, np.exp(2 * _SIDE_ETA * _SIDE_POS + 1j * _SIDE_ARG)),
        _case("K4_left", 0, 200, (-9, -1), SIDE_BS, np.exp(-2 * _SIDE_ETA * _SIDE_POS + 1j * _SIDE_ARG)),
        _case("K2_D2", 0, 2, (-1, 1), K4_BS[:2], K4_NC[:2]),
        _case("K2_D3", 0, 3, (-1, 1), K4_BS[:2], K4_NC[:2]),            # t = 0 is sample 1
        _case("K2_D513", 0, 513, (-12, 12), K4_BS[:2], K4_NC[:2]),      # one lane of a third workgroup; t = 0 is sample 256
        _case("K4_residues", 0, 64, (-12, 12), K4_BS, IC._nc_to_residues(K4_BS, K4_NC), RESIDUES),
        _case("K4_unsorted", 0, 64, (-12, 12), K4_BS[[2, 0, 3, 1]], K4_NC[[2, 0, 3, 1]]),
    ]
    m1 = [_case("chirp_K4_D%d" % D, 1, D, (-1, 1) if D <= 10 else (-12, 12), K4_BS, K4_NC, seed="chirp")
          for D in (2, 3, 9, 10, 64, 300)]
    m1 += [_case("chirp_K2_D%d" % D, 1, D, (-12, 12), K4_BS[:2], K4_NC[:2], seed="chirp") for D in (2048, 2049, 2050)]
    m1 += [
        _case("addsoliton_D64", 1, 64, add[64]["T"], add[64]["bound_states"], add[64]["normconsts"], seed="addsoliton"),
        _case("addsoliton_D512", 1, 512, add[512]["T"], add[512]["bound_states"], add[512]["normconsts"],
              seed="addsoliton"),
        _case("zero_K3", 1, 128, (-12, 12), K4_BS[:3], K4_NC[:3], seed="zero"),
        _case("gap_K4", 1, 64, (-12, 12), K4_BS, K4_NC, seed="gap"),
        _case("chirp_K8", 1, 128, (-12, 12), K8_BS, K8_NC, seed="chirp"),
        _case("chirp_K4_residues", 1, 64, (-12, 12), K4_BS[[2, 0, 3, 1]], IC._nc_to_residues(K4_BS, K4_NC)[[2, 0, 3, 1]],
              RESIDUES, seed="chirp"),
        _case("chirp_K4_offzero", 1, 64, (0.5, 12.5), K4_BS, K4_NC, seed="chirp"),
        # ks = -|q|^2 - lambda^2 == 0 exactly on the plateau |t| < 2
        _case("ks_zero_tails", 1, 300, (-12, 12), [0.5j], [0.3], seed="plateau"),
        _case("ks_zero_K2", 1, 300, (-12, 12), [0.5j, 0.3 + 0.9j], [0.3, -1.1j], seed="plateau"),
    ]
    return m0 + m1


def seed_samples(c):
    """The seed potential of a mode-1 case in double (the kernels and the reference both start from these)."""
    D, T = c["D"], c["T"]
    t = IC.tgrid(T, D)
    name = c["seed"]
    if name == "zero":
        return np.zeros(D, np.complex128)
    if name == "addsoliton":
        return -0.4 * IC.sech(t) * np.exp(-5j * t)
    if name == "plateau":          # 0.5 on |t| < 2, tails 0.2 sech(t)
        return np.where(np.abs(t) < 2, 0.5, 0.2 * IC.sech(t)).astype(np.complex128)
    q = 0.7 * IC.sech(t - 1) * np.exp(1j * (0.2 * t * t + 0.5 * t))
    if name == "gap":              # a run of exact zeros
        q = np.where((t > -2) & (t < 0.5), 0.0, q)
    else:
        assert name == "chirp", name
    return q * c.get("seed_scale", 1.0)


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}
# the (D, K) groups whose batch of three runs: every workgroup count of the sample kernels, the chunk layouts, both modes
# and both kinds of constants.  The plan exists for the powers of two only; the emulator runs them all.
BATCH_GROUPS = ("K1", "K16_wide", "K3_hugeb", "K2_D2", "K4_residues", "chirp_K4_D2", "chirp_K4_D10", "chirp_K4_D64",
                "chirp_K4_D300", "chirp_K2_D2048", "chirp_K2_D2050", "addsoliton_D512", "chirp_K4_residues",
                "ks_zero_K2")


def case_ids(cases=None):
    return [c["id"] for c in (CASES if cases is None else cases)]


def power_of_two(c):
    return c["D"] & (c["D"] - 1) == 0


def batch_signals(c):
    """Three different signals of the case's (D, K) group: the case; its bound states in reverse order with other
    constants; bound states moved along the real axis, other constants, the seed scaled.  Each is a case of its own."""
    bs, nc = np.asarray(c["bs"]), np.asarray(c["nc"])
    b = dict(c, id=c["id"] + "#rev", bs=_c(bs[::-1]), nc=_c(nc[::-1] * (0.8 * np.exp(0.5j))))
    d = dict(c, id=c["id"] + "#moved", bs=_c(bs + 0.05), nc=_c(nc * (1.3 * np.exp(-0.4j))), seed_scale=0.9)
    return [c, b, d]


# ---- the double-precision yardsticks ----------------------------------------------------------------------------------
def _opts(c):
    return dict(discspec_type=c["dstype"],
                contspec_inversion_method="USE_SEED_POTENTIAL_INSTEAD" if c["mode"] else "DEFAULT")


def oracle_double(c, skip_ks_zero=True):
    """e1's run: oracle.inverse.add_discrete_spectrum, the reference restated in double.  skip_ks_zero=False: a copy of
    its integrator (the half steps in sequence, the inverse steps as adjugate over determinant) with the limit
    sinh(k h)/k -> h at ks == 0 instead of the reference's skipped step."""
    if skip_ks_zero:
        from oracle.inverse import add_discrete_spectrum
        q = seed_samples(c) if c["mode"] else np.zeros(c["D"], np.complex128)
        rc = add_discrete_spectrum(c["bs"], c["nc"], q, list(c["T"]), 0, _opts(c))
        assert rc == 0, (c["id"], rc)
        return q
    assert c["mode"] == 1
    bs, nc = R.prepared(c["bs"], c["nc"], c["dstype"] == RESIDUES, np.complex128)
    q = seed_samples(c)
    D, T = c["D"], c["T"]
    ch, sh = R.step_coefficients(bs, q, ((T[1] - T[0]) / (D - 1)) / 2, np.complex128)
    u1 = 1j * bs[:, None] * sh
    K = bs.size
    phi, psi = np.zeros((K, 2, D), np.complex128), np.zeros((K, 2, D), np.complex128)
    p1, p2 = np.exp(-1j * bs * T[0]), np.zeros(K, np.complex128)
    phi[:, 0, 0], phi[:, 1, 0] = p1, p2
    for n in range(1, D):
        for m in (n - 1, n):
            p1, p2 = ((ch[:, m] - u1[:, m]) * p1 + q[m] * sh[:, m] * p2,
                      -np.conj(q[m]) * sh[:, m] * p1 + (ch[:, m] + u1[:, m]) * p2)
        phi[:, 0, n], phi[:, 1, n] = p1, p2
    s1, s2 = np.zeros(K, np.complex128), np.exp(1j * bs * T[1])
    psi[:, 0, D - 1], psi[:, 1, D - 1] = s1, s2
    for n in range(D - 1, 0, -1):
        for m in (n, n - 1):
            scl = (ch[:, m] - u1[:, m]) * (ch[:, m] + u1[:, m]) - (-np.conj(q[m]) * sh[:, m]) * (q[m] * sh[:, m])
            s1, s2 = (((ch[:, m] + u1[:, m]) * s1 - q[m] * sh[:, m] * s2) / scl,
                      (np.conj(q[m]) * sh[:, m] * s1 + (ch[:, m] - u1[:, m]) * s2) / scl)
        psi[:, 0, n - 1], psi[:, 1, n - 1] = s1, s2
    return R.cdt_steps(bs, nc, q, phi, psi, np.complex128)


def second_association(c):
    """e2's run, in double.  Mode 1: the eigenfunctions from chunk maps of 16 half-step samples composed as
    body_bs_combine composes them, the backward steps as exp(-A h) (darboux_ref.eigenfunctions_chunked).  Mode 0: the
    recursion on the grid t_n rounded once from long double (what a fused T0 + eps_t n gives) instead of the double
    product and sum."""
    bs, nc = R.prepared(c["bs"], c["nc"], c["dstype"] == RESIDUES, np.complex128)
    if c["mode"] == 0:
        _, t, _ = R.grid(c["T"], c["D"])
        return R.solitons_ref(bs, nc, c["T"], c["D"], np.complex128, t=t.astype(np.float64))
    q = seed_samples(c)
    with np.errstate(over="ignore", invalid="ignore"):
        phi, psi = R.eigenfunctions_chunked(bs, q, c["T"], np.complex128)
        return R.cdt_steps(bs, nc, q, phi, psi, np.complex128)


def reference(c, nc_factor=None):
    """The long-double answer of the case.  nc_factor = (k, f): the caller's constant number k times f (sensitivity)."""
    nc = np.array(c["nc"])
    if nc_factor is not None:
        nc[nc_factor[0]] *= nc_factor[1]
    bs, ncs = R.prepared(c["bs"], nc, c["dstype"] == RESIDUES)
    if c["mode"] == 0:
        return R.solitons_ref(bs, ncs, c["T"], c["D"])
    e = _eigen(c["id"], c)
    return R.cdt_steps(bs, ncs, seed_samples(c), e[0], e[1])


_EIGEN = {}


def _eigen(cid, c):
    """phi, psi of the seed at the sorted bound states (they do not depend on the constants), once per process."""
    if cid not in _EIGEN:
        bs, _ = R.prepared(c["bs"], c["nc"], False)
        with np.errstate(over="ignore", invalid="ignore"):
            _EIGEN[cid] = R.eigenfunctions_ref(bs, seed_samples(c), c["T"])
    return _EIGEN[cid]


_EVAL = {}


def evaluated(c):
    """Of a case (of the table or of batch_signals): q_ref (long double, read-only) and the errors against it of the two
    double-precision yardsticks -- e1, oracle.inverse.add_discrete_spectrum (for the ks_zero cases its integrator with
    the limit: the reference's skipped step is a different function there, see test_darboux_cases_cpu), and e2, the
    second association -- and Y = max(4 u, e1, e2).  Computed once per process."""
    cid = c["id"]
    if cid not in _EVAL:
        q_ref = reference(c)
        assert np.all(np.isfinite(q_ref)), cid
        q_ref.setflags(write=False)
        e1 = R.error(oracle_double(c, skip_ks_zero=not cid.startswith("ks_zero")), q_ref)
        e2 = R.error(second_association(c), q_ref)
        _EVAL[cid] = dict(q_ref=q_ref, e1=e1, e2=e2, Y=max(Y_FLOOR, e1, e2))
    return _EVAL[cid]


def Y(c):
    return evaluated(c)["Y"]


def bound(c):
    return FACTOR * Y(c)
