"""Inputs of the Richardson tests of the batched nsev plans that the emulator tests (test_richardson_emu.py) and the GPU
tests (test_gpu_nsev_batch_richardson.py) share: small sech pulses on a wide xi-grid, so that the grid points with
|xi| < 0.9 pi / (2 eps_t_sub) -- the ones fnft_nsev extrapolates -- are a proper subset of the grid."""
import numpy as np

import signals as S

CS_T, CS_XI, CS_M = (-8.0, 8.0), (-4.0, 4.0), 48
CS_AMPS = (1.3, 0.8)
# (scheme, D, first and last index of the extrapolated grid points: the oracle's own set)
CS_CASES = [("2SPLIT2A", 64, 8, 39), ("4SPLIT4B", 64, 8, 39), ("2SPLIT4B", 65, 7, 40)]
CS_TYPES = [("BOTH", "BOTH", 2, 3), ("REFLECTION_COEFFICIENT", "RHO", 0, 1)]     # capi name, oracle name, code, parts


def cs_signals(D):
    return np.stack([S.sech_focusing(D, CS_T, amp=a) for a in CS_AMPS])
