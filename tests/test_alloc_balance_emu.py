"""Every plan class allocates through one arena (fnft_amd/csrc/nft_arena.h).  Over a back end that counts
(tests/emu/emu_alloc_balance.cpp), for the smallest shapes that reach every allocation branch of the init() functions:
a successful init() followed by the end of the plan's scope leaves no block behind, and the plan's byte count is what the
back end saw requested; an init() that finds no memory at its n-th request, for every n, returns an error and leaves no
block behind either, and no block is ever handed back twice.  The parts a plan is made of (twiddle tables, any-length
DFT, resampler: fnft_amd/csrc/nft_twiddles.h, nft_chirp.h) stand alone under the same assertions, and a tree plan on
borrowed tables requests what the owning plan requests minus the tables.
The discrete-spectrum plan (nft_discspec_plan.h) stands under them with its Richardson stage enabled, as a guess plan
and as a guess-free one: enable_richardson() failing at any request leaves no block behind and the plan as it was.
The same library records the launches of one run() of the batched plan classes (emu_plan_schedule): which kernels the
parts contribute to them, and that a call with the stage is the plain call followed by the coarse pass and one match
kernel.  No kernel executes.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fnft_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libfnft_emu_alloc_balance.so")
CSRC = os.path.join(ROOT, "fnft_amd", "csrc")

PLAN, SLOW, DISCSPEC, INVERSE, RESAMPLER, ANYDFT, PLAN_BORROWED, DISCSPEC_PLAN = 0, 1, 2, 3, 4, 5, 6, 7
D = capi.NSE_DISC
CASES = {
    # NftPlan: D of the tree, M, batch, akns discretization, its degree, input samples, upsampling, kdv
    "plan-2SPLIT2_MODAL": (PLAN, [64, 16, 2, 0, 1, 64, 1, 0]),
    "plan-4SPLIT4B-resampler": (PLAN, [128, 16, 1, 10, 2, 64, 2, 0]),          # akns 4B: degree 2
    "plan-2SPLIT8B-kdv": (PLAN, [64, 16, 1, 18, 12, 64, 1, 1]),                # akns 8B: degree 12, coefficient program
    # NftSlowPlan: D, M, batch, discretization, contspec type, Richardson
    "slow-CF4_2-front-richardson": (SLOW, [64, 16, 2, D["CF4_2"], 2, 1]),      # 64 samples: the transform resampler
    "slow-BO-reduce": (SLOW, [4096, 16, 1, D["BO"], 2, 0]),                    # >= 64 chunks: the reduce stage's buffers
    # NftDiscSpecBatch: D, K, batch, discretization
    "discspec-4SPLIT4B": (DISCSPEC, [64, 3, 2, D["4SPLIT4B"]]),
    # NftDiscSpecPlan: D, K, batch, discretization, localization (1: guess plan, 2: guess-free), Richardson stage enabled
    "discspec-plan-4SPLIT4B-guess-richardson": (DISCSPEC_PLAN, [64, 3, 2, D["4SPLIT4B"], 1, 1]),
    "discspec-plan-2SPLIT2A-search-richardson": (DISCSPEC_PLAN, [64, 3, 2, D["2SPLIT2A"], 2, 1]),
    # NftInverseBatch: D, M, batch, cstype, oversampling, modal, K, discrete mode, residues
    "inverse-b-of-xi-K2": (INVERSE, [512, 512, 2, 1, 8, 1, 2, 1, 1]),          # 512 > leaf: work arrays and sub-plans
    "inverse-M0-K2": (INVERSE, [512, 0, 2, 0, 8, 1, 2, 0, 0]),
    # NftResampler alone (with the tables it borrows in the same arena): input samples, batch
    "resampler-D64-batch2": (RESAMPLER, [64, 2]),
    # NftAnyDft alone: largest length, transforms at a time (37: the shortest chirp, 4099: a prime above 4096)
    "anydft-37": (ANYDFT, [37, 2]),
    "anydft-4099": (ANYDFT, [4099, 2]),
}
# NftPlan on tables it borrows: the arguments of the owning case
BORROWED = {"plan-borrowed-" + k[5:]: (PLAN_BORROWED, v[1]) for k, v in CASES.items() if v[0] == PLAN}
CASES.update(BORROWED)
# bytes of one set of twiddle tables without the lengths 3*2^b, with them (nft_twiddles.h)
TABLES = 16 * (2 * 16384 + 2 ** 12 + 2 ** 13)
TABLES3 = TABLES + 16 * (3 * 2 ** 13 + 2 ** 12)


@pytest.fixture(scope="module")
def emu():
    deps = [os.path.join(EMU_DIR, f) for f in ("emu_alloc_balance.cpp", "emu_backend.h")]
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(EMU_LIB) or max(map(os.path.getmtime, deps)) > os.path.getmtime(EMU_LIB):
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas",
                               "-o", EMU_LIB, os.path.join(EMU_DIR, "emu_alloc_balance.cpp")])
    L = C.CDLL(EMU_LIB)
    L.emu_alloc_balance.argtypes = [C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    L.emu_plan_schedule.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    return L


def run(emu, kind, args, fail_at):
    a = np.array(args, np.int64)
    out = np.zeros(6, np.uint64)
    rc = emu.emu_alloc_balance(kind, a.ctypes.data_as(C.c_void_p), fail_at, out.ctypes.data_as(C.c_void_p))
    return (rc,) + tuple(int(x) for x in out)


@pytest.mark.parametrize("case", sorted(CASES))
def test_arena_balances(emu, case):
    kind, args = CASES[case]
    rc, nalloc, live, requested, class_bytes, bad, _ = run(emu, kind, args, -1)
    print(case, "requests", nalloc, "bytes", requested)
    assert rc == 0
    assert nalloc > 0 and live == 0 and bad == 0
    assert class_bytes == requested
    for n in range(nalloc):
        rc, _, live, _, _, bad, extra = run(emu, kind, args, n)
        assert rc != 0, (case, n)
        assert live == 0 and bad == 0, (case, n, live, bad)
        if kind == DISCSPEC_PLAN:      # a failing enable_richardson(): no block behind while the plan lives, and it still runs
            assert extra == 0, (case, n, extra)


@pytest.mark.parametrize("case", sorted(k for k, v in CASES.items() if v[0] == DISCSPEC_PLAN))
def test_enable_richardson_fails_at_every_request(emu, case):
    """The requests of enable_richardson() alone (those after init()'s): each in turn finds no memory."""
    kind, args = CASES[case]
    plain = run(emu, kind, args[:5] + [0], -1)
    full = run(emu, kind, args, -1)
    assert plain[0] == 0 and full[0] == 0 and full[1] > plain[1] and full[3] > plain[3]
    for n in range(plain[1], full[1]):
        rc, _, live, requested, class_bytes, bad, extra = run(emu, kind, args, n)
        assert rc != 0 and live == 0 and bad == 0 and extra == 0, (case, n, rc, live, bad, extra)
        assert class_bytes == plain[4] == plain[3]     # the plan's count is that of the plan without the stage
        assert requested >= plain[3]                   # init() was served in full


@pytest.mark.parametrize("case", sorted(BORROWED))
def test_borrowed_tables(emu, case):
    """The plan on borrowed tables requests exactly the owning plan's bytes minus the tables."""
    own = run(emu, PLAN, BORROWED[case][1], -1)
    rc, _, _, requested, _, _, plan_bytes = run(emu, *BORROWED[case], -1)
    tables = TABLES3 if BORROWED[case][1][7] else TABLES
    print(case, "owning plan", own[3], "borrowing plan", plan_bytes, "tables", tables)
    assert rc == 0 and own[0] == 0
    assert requested == own[3]                  # tables in the owner's arena + the plan = the owning plan
    assert plan_bytes == own[3] - tables


# ---- launches of one run() of the batched plan classes -----------------------------------------------------------------
def schedule(emu, kind, args):
    a = np.array(args, np.int64)
    buf = C.create_string_buffer(1 << 18)
    rc = emu.emu_plan_schedule(kind, a.ctypes.data_as(C.c_void_p), buf, len(buf))
    assert rc == 0, (kind, args, rc)
    return [n.replace(" ", "") for n in buf.value.decode().split("\n") if n]


def chirp_kinds(names):
    """(kernel, column length, DFT mode) of every chirp column kernel; KChirpRows as it is."""
    out = []
    for n in names:
        m = re.match(r"^(KChirpColFwd|KChirpColInv)<(\d+),(true|false)", n)
        if m:
            out.append((m.group(1), int(m.group(2)), m.group(3) == "true"))
        elif n == "KChirpRows":
            out.append((n, 0, True))
    return out


DFT_TRIPLE = ["KChirpColFwd", "KChirpRows", "KChirpColInv"]


def test_discspec_front_is_the_resampler_alone(emu):
    """NftDiscSpecBatch, 4SPLIT4B: the front end is the resampler and the combination, and no level 0 of a tree."""
    names = schedule(emu, DISCSPEC, CASES["discspec-4SPLIT4B"][1])
    front = names[:names.index("KDsBox")]
    assert [k for k, _, dft in chirp_kinds(front)] == DFT_TRIPLE * 2 and all(d for _, _, d in chirp_kinds(front))
    rest = [n for n in front if not n.startswith("KChirp")]
    assert rest == ["KBandCheck", "KResamplePhase", "KResampleCombine"], front
    assert front.index("KBandCheck") == 3 and front[-1] == "KResampleCombine"
    assert not [n for n in names if n.startswith(("KCoeffs", "KLeaf"))], names


def test_slow_second_pass_reuses_the_spectrum(emu):
    """NftSlowPlan, CF4_2 with Richardson: the first pass transforms the signal and checks its band, the second (every
    other sample, fwd = false) starts at the phase ramps."""
    names = schedule(emu, SLOW, CASES["slow-CF4_2-front-richardson"][1])
    cut = [i for i, n in enumerate(names) if n == "KSlowPrep"]
    assert len(cut) == 2
    first, second = names[:cut[0]], names[cut[0] + 1:cut[1]]
    second = second[next(i for i, n in enumerate(second) if n.startswith(("KChirp", "KResample", "KBandCheck"))):]
    assert [k for k, _, _ in chirp_kinds(first)] == DFT_TRIPLE * 2
    assert [n for n in first if not n.startswith("KChirp")] == ["KBandCheck", "KResamplePhase"]
    assert [k for k, _, _ in chirp_kinds(second)] == DFT_TRIPLE
    assert [n for n in second if not n.startswith("KChirp")] == ["KResamplePhase"] and second[0] == "KResamplePhase"


def test_inverse_dfts_run_at_their_own_length(emu):
    """NftInverseBatch, b(xi), D = M = 512, oversampling 8: the M-point DFT and the four of the spectral factorization
    (next_fast_size(513 * 8) = 4104 points) each run at the column length NftAnyDft::len(n) / kRowChirp of their own length, not at
    the workspace's."""
    names = schedule(emu, INVERSE, [512, 512, 2, 1, 8, 1, 0, 0, 0])
    row = 4096                                                    # kRowChirp (tests/chirp_cases.py: ROW)

    def n1(n):
        L = 1
        while L < 2 * n - 1:
            L *= 2
        return max(L, 2 * row) // row
    ck = chirp_kinds(names)
    assert [k for k, _, _ in ck] == DFT_TRIPLE * 5 and all(d for _, _, d in ck)
    want = [n1(512)] + [n1(4104)] * 4
    assert [c for k, c, _ in ck if k == "KChirpColFwd"] == want
    assert [c for k, c, _ in ck if k == "KChirpColInv"] == want
    assert n1(512) != n1(4104)


# ---- the discrete-spectrum plan: one statement of "fine pass, then stage" ------------------------------------------------
DS_PLAN = [64, 3, 2]                                               # D, K, batch
COARSE_TAIL = ["KDsBox", "KDsNewton", "KDsFilter", "KDsNorm", "KRichMatchDs"]


def base(names):
    """kernel names without their template arguments"""
    return [n.split("<")[0] for n in names]


@pytest.mark.parametrize("disc,bsloc,front", [("4SPLIT4B", 1, "resampler"), ("2SPLIT2A", 2, "gather")])
def test_discspec_plan_schedules(emu, disc, bsloc, front):
    """NftDiscSpecPlan, guess plan and guess-free plan: with the stage, a call is the plain call followed by the coarse
    front (KDsGather, or the resampler's launches), the coarse pass's box, Newton, filter and norming kernels and one
    KRichMatchDs, last.  The guess plan's plain call is NftDiscSpecBatch's."""
    plain = schedule(emu, DISCSPEC_PLAN, DS_PLAN + [D[disc], bsloc, 0])
    rich = schedule(emu, DISCSPEC_PLAN, DS_PLAN + [D[disc], bsloc, 1])
    if bsloc == 1:
        assert plain == schedule(emu, DISCSPEC, DS_PLAN + [D[disc]])
    else:
        assert "KDsCandidates" in plain and "KAberthBStart" in plain
    assert rich[:len(plain)] == plain and "KRichMatchDs" not in plain
    tail = rich[len(plain):]
    cut = tail.index("KDsBox")
    coarse_front, coarse = tail[:cut], tail[cut:]
    if front == "gather":
        assert coarse_front == ["KDsGather"]
    else:       # the resampler over all D samples: forward DFT, band check, phase ramps, inverse DFTs, combination
        assert [k for k, _, _ in chirp_kinds(coarse_front)] == DFT_TRIPLE * 2
        assert [n for n in coarse_front if not n.startswith("KChirp")] == ["KBandCheck", "KResamplePhase", "KResampleCombine"]
    assert base(coarse) == COARSE_TAIL, coarse
    assert rich.count("KRichMatchDs") == 1 and rich[-1] == "KRichMatchDs"
