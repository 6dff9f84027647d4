"""Case table and inputs of the layer-peeling path tests (tests/test_peel_cases_cpu.py, tests/test_gpu_peel_paths.py).

A case is a transfer matrix of D samples, a sign kappa and one of the two discretizations with a base case.  The
inputs are chosen as step parameters Q_n = eps_t q(t_n), so one table serves both discretizations: the transfer matrix
is the product of the steps scl_n [[1, Q_n z], [-kappa Q_n*, z]], scl_n = 1/sqrt(1 + kappa |Q_n|^2), the last sample
leftmost, formed in double by an FFT product tree (the arithmetic of oracle.oracle._conv2x2).  It need not be exact:
the reference (tests/peel_ref.py) starts from the same doubles as the kernels.

Signals on T = [-8, 8], eps = 16/(D - 1), t_n = -8 + n eps, |Q_n| clipped to 0.7:
  a06    q = 0.6 sech(t) exp(i (0.3 t^2 + 0.7 t + 0.4))
  a10    the same with amplitude 1.0: L1 norm pi, the strongest coupling used (the error of peeling grows like
         exp(2 ||q||_1): it is the L1 norm sum |Q_n|, not the energy, that conditions the problem)
  rough  a06 times 1 + 0.3 (g1 + i g2) per sample, g from default_rng(crc32(case id))
  steps  D <= 32 only: Q_n = min(0.6, 2.4/D) exp(i (1.1 n + 0.3)) -- the sech signals put next to nothing on 2 or 8
         samples of [-8, 8], this one gives the short leaf paths large |Q|

Sizes: the smallest D at which each path of NftLayerPeelingDev::peel / prod first runs (PATHS below), every kappa,
discretization and signal up to D = 1024, two combinations above, one at D = 16384.
"""
import functools
import zlib

import numpy as np

import peel_ref as R

U = R.U
T = (-8.0, 8.0)
MODAL, A2 = "2SPLIT2_MODAL", "2SPLIT2A"

# the GPU's error may be FACTOR times the larger CPU yardstick of its group (D, kappa) -- see bound().  What differs
# legitimately between numpy and the kernels (FFT radix and twiddle tables, fused multiply-adds, a reciprocal from an
# approximation and two Newton steps instead of a division) changes the error by small constant factors, never its
# growth with D.  Largest measured e_gpu / Y per D on an MI355X (profiles/peel_errors.json; scaling, resident-state and
# after-failure calls included):
#   D      2     4     8     16    32    64    128   256   512   1024  2048  4096  8192  16384
#   ratio  0.67  1.03  0.91  0.68  0.77  2.51  1.73  1.33  0.64  1.41  0.76  0.61  0.30  0.49
# Tried against this bound with deliberately wrong builds: the aliased top coefficient of KPeelProduct left unfolded
# fails D = 1024 (ratio 8e13; at D = 512 the product's coefficient 0 is never read).  Two changes stay below it: the
# leaf's reciprocal with one Newton step instead of two (an error of a few 2^-50 per step: at D = 4 the largest e_gpu
# goes from 4.5 u to 15.8 u, ratio 1.03 to 3.66, where the bound is at its floor of 8 * 4 u; from D = 64 on it drowns
# in the accumulated rounding), and the leaf's inverse without its factor S (a common scalar factor of a transfer
# matrix never changes the samples: S only keeps the magnitudes in range; D = 512 stays at ratio 0.64).
FACTOR = 8.0
Y_FLOOR = 4 * U

# ---- paths ----------------------------------------------------------------------------------------------------------
# per D: the peeling kernels of the library's instantiation list the call launches, and the products that go through a
# resident plan (KPeelImport, an n = 2 tree of that degree, the strided export) as "plan<degree>:step<2|4>"
_P512, _P1024, _P2048 = "KPeelProduct<512>", "KPeelProduct<1024>", "KPeelProduct<2048>"
PATHS = {
    # leaf alone, Ti = NULL: d = 2 is the branch with the constant terms outside slot 3; 4 .. 128 the slot-3 branch with
    # 1 .. 32 active lanes and a partial last visit of the four-step fetch of Q (d = 4: exactly one visit); 256 full
    2: (["KPeelLeaf"], []), 4: (["KPeelLeaf"], []), 8: (["KPeelLeaf"], []), 16: (["KPeelLeaf"], []),
    32: (["KPeelLeaf"], []), 64: (["KPeelLeaf"], []), 128: (["KPeelLeaf"], []), 256: (["KPeelLeaf"], []),
    # leaf with Ti != NULL (both columns of the inverse, the product of the scale factors), step 2 in one launch
    512: (["KPeelLeaf", _P1024], []),
    # step 4 (degree 256, strided output into the parent's T2i + h)
    1024: (["KPeelLeaf", _P2048, _P1024, _P512], []),
    # step 2 through a plan; step 4 at degree 512
    2048: (["KPeelLeaf", "KPeelImport", _P2048, _P1024, _P512], ["plan2048:step2"]),
    # step 4 at degree 1024, plan product of degree 4096
    4096: (["KPeelLeaf", "KPeelImport", _P2048, _P1024, _P512], ["plan4096:step2", "plan2048:step2"]),
    # step 4 through a plan (degree 2048, output into the parent's T2i + h)
    8192: (["KPeelLeaf", "KPeelImport", _P2048, _P1024, _P512],
           ["plan8192:step2", "plan4096:step2", "plan2048:step2", "plan2048:step4"]),
    # step 4 through a plan of degree 4096
    16384: (["KPeelLeaf", "KPeelImport", _P2048, _P1024, _P512],
            ["plan16384:step2", "plan8192:step2", "plan4096:step2", "plan2048:step2", "plan2048:step4",
             "plan4096:step4"]),
}
PEEL_PREFIX = "KPeel"


def case_id(D, signal, kappa, disc):
    return "D%d_%s_k%s_%s" % (D, signal, "p" if kappa > 0 else "m", "modal" if disc == MODAL else "2A")


def make_case(D, signal, kappa, disc):
    return dict(id=case_id(D, signal, kappa, disc), D=D, signal=signal, kappa=kappa, disc=disc, eps_t=16.0 / (D - 1),
                kernels=PATHS[D][0], paths=PATHS[D][1])


def _table():
    cases = []
    for D in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        for signal in ("a06", "a10", "rough") + (("steps",) if D <= 32 else ()):
            for kappa in (1, -1):
                for disc in (MODAL, A2):
                    cases.append(make_case(D, signal, kappa, disc))
    for D in (2048, 4096, 8192):
        for signal in ("a10", "rough"):
            cases.append(make_case(D, signal, 1, A2))
            cases.append(make_case(D, signal, -1, MODAL))
    cases.append(make_case(16384, "a10", -1, A2))
    return cases


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}


def case_ids():
    return [c["id"] for c in CASES]


def groups():
    return sorted({(c["D"], c["kappa"]) for c in CASES})


# ---- inputs ---------------------------------------------------------------------------------------------------------
def step_parameters(c):
    """Q_n of the case, n = 0 .. D-1."""
    D = c["D"]
    n = np.arange(D)
    if c["signal"] == "steps":
        assert D <= 32
        return min(0.6, 2.4 / D) * np.exp(1j * (1.1 * n + 0.3))
    eps = (T[1] - T[0]) / (D - 1)
    t = T[0] + n * eps
    amp = 1.0 if c["signal"] == "a10" else 0.6
    q = amp / np.cosh(t) * np.exp(1j * (0.3 * t * t + 0.7 * t + 0.4))
    if c["signal"] == "rough":
        rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
        g1, g2 = rng.standard_normal(D), rng.standard_normal(D)
        q = q * (1 + 0.3 * (g1 + 1j * g2))
    Q = eps * q
    a = np.abs(Q)
    return Q * (np.minimum(a, 0.7) / np.maximum(a, 1e-300))


def transfer_matrix(Q, kappa, scl=None):
    """tm [4, D+1] (entries 11, 12, 21, 22, highest power first) of the steps Q_n in double: a product tree, every level
    one batched FFT convolution of 2x2 polynomial matrices (the later samples on the left)."""
    Q = np.asarray(Q, np.complex128)
    D = Q.size
    assert D >= 2 and D & (D - 1) == 0
    if scl is None:
        scl = 1.0 / np.sqrt(1.0 + kappa * np.abs(Q) ** 2)
    M = np.zeros((D, 4, 2), np.complex128)
    M[:, 0, 1] = scl
    M[:, 1, 0] = scl * Q
    M[:, 2, 1] = -scl * kappa * np.conj(Q)
    M[:, 3, 0] = scl
    while M.shape[0] > 1:
        A, B = M[1::2], M[0::2]
        n = 2 * A.shape[2] - 1
        L = 1 << int(np.ceil(np.log2(n)))
        FA, FB = np.fft.fft(A, L, axis=2), np.fft.fft(B, L, axis=2)
        FC = np.stack([FA[:, 0] * FB[:, 0] + FA[:, 1] * FB[:, 2], FA[:, 0] * FB[:, 1] + FA[:, 1] * FB[:, 3],
                       FA[:, 2] * FB[:, 0] + FA[:, 3] * FB[:, 2], FA[:, 2] * FB[:, 1] + FA[:, 3] * FB[:, 3]], axis=1)
        M = np.fft.ifft(FC, axis=2)[:, :, :n]
    return np.ascontiguousarray(M[0])


def failing_transfer_matrix(D=1024, n_bad=700):
    """kappa = -1 and one |Q_n| = 1.05 among the steps of a06: sample n_bad violates 1 - |Q|^2 > 0, which the peeling
    has to report (:173-176).  scl from |1 - |Q|^2| keeps the matrix finite.  -> (tm, eps_t)"""
    c = make_case(D, "a06", -1, MODAL)
    Q = step_parameters(c)
    Q[n_bad] = 1.05 * np.exp(0.5j)
    return transfer_matrix(Q, -1, 1.0 / np.sqrt(np.abs(1.0 - np.abs(Q) ** 2))), c["eps_t"]


# ---- reference and yardsticks, computed once per process ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _evaluated(cid, D, signal, kappa, disc):
    from oracle.oracle import nse_finvscatter
    c = make_case(D, signal, kappa, disc)
    assert c["id"] == cid
    Q = step_parameters(c)
    tm = transfer_matrix(Q, kappa)
    rc, q_ref = R.peel(tm, c["eps_t"], kappa, disc)
    assert rc == 0, cid
    rc, q_seq = R.peel(tm, c["eps_t"], kappa, disc, np.complex128)
    assert rc == 0, cid
    rc, q_rec = nse_finvscatter(tm, c["eps_t"], kappa, disc)
    assert rc == 0, cid
    for a in (tm, q_ref):
        a.setflags(write=False)
    return dict(tm=tm, q_ref=q_ref, q_constructed=R.samples(Q, c["eps_t"], disc), e_seq=R.error(q_seq, q_ref),
                e_rec=R.error(q_rec, q_ref))


def evaluated(c):
    """Of a case (of the table or of make_case): tm (double, read-only), q_ref (long double, read-only), q_constructed
    (the samples the steps were built from) and the errors of the two double-precision yardsticks against q_ref --
    e_seq, the sequential loop of peel_ref.py in complex128, and e_rec, oracle.oracle.nse_finvscatter (the reference's
    recursion with FFT products)."""
    return _evaluated(c["id"], c["D"], c["signal"], c["kappa"], c["disc"])


@functools.lru_cache(maxsize=None)
def Y(D, kappa):
    """The larger yardstick over every case of the table with this D and kappa (the maximum over the group evens out
    one case that is accurate by chance), at least 4 u."""
    es = [max(evaluated(c)["e_seq"], evaluated(c)["e_rec"]) for c in CASES if c["D"] == D and c["kappa"] == kappa]
    assert es, (D, kappa)
    return max(Y_FLOOR, max(es))


def bound(c):
    return FACTOR * Y(c["D"], c["kappa"])
