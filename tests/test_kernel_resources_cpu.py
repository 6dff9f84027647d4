"""Registers of the product tree's row kernels (`KMidSym`) and fused-level kernels (`KMulti`), without a GPU: each runs at
two waves per SIMD with no VGPR spilled and no scratch.  The figures are the code-object metadata of the built library
(fnft_amd/lib/libfnft_amd.so, what `hipcc -Rpass-analysis=kernel-resource-usage` reports), read with the ROCm LLVM tools.
A spill of these kernels is HBM traffic on the headline path (0.25 GB per cfg 2 step before they were made spill-free)."""
import os

import pytest

from kernel_notes import LIB, kernel_resources

# symbol of kernel_entry<K> -> K
KERNELS = {
    "_Z12kernel_entryI7KMidSymILb1EEEvNT_6ParamsE": "KMidSym<true>",
    "_Z12kernel_entryI7KMidSymILb0EEEvNT_6ParamsE": "KMidSym<false>",
    "_Z12kernel_entryI6KMultiILi1024ELi3EEEvNT_6ParamsE": "KMulti<1024, 3>",
    "_Z12kernel_entryI6KMultiILi128ELi3EEEvNT_6ParamsE": "KMulti<128, 3>",
    "_Z12kernel_entryI6KMultiILi1024ELi2EEEvNT_6ParamsE": "KMulti<1024, 2>",
    "_Z12kernel_entryI6KMultiILi128ELi2EEEvNT_6ParamsE": "KMulti<128, 2>",
}
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size")


def waves_per_simd(vgpr, agpr):
    """Waves per SIMD the registers allow on gfx950: one file of 512 registers per lane for VGPRs and AGPRs, allocated
    in granules of 8 (AGPRs start at a multiple of 4)."""
    total = (-(-vgpr // 4) * 4 + agpr) if agpr else vgpr
    return min(8, 512 // (-(-total // 8) * 8))


@pytest.fixture(scope="module")
def resources():
    assert os.path.exists(LIB), "libfnft_amd.so is not built (python -m fnft_amd.build)"
    return kernel_resources(KERNELS, KEYS)


@pytest.mark.parametrize("kernel", sorted(KERNELS.values()))
def test_no_spill_two_waves(resources, kernel):
    r = resources.get(kernel)
    assert r is not None and all(k in r for k in KEYS), (kernel, r)
    assert r["vgpr_spill_count"] == 0, (kernel, r)
    assert r["private_segment_fixed_size"] == 0, (kernel, r)
    assert waves_per_simd(r["vgpr_count"], r["agpr_count"]) >= 2, (kernel, r)


def test_waves_per_simd_table():
    # MI355X register table: 176-256 registers per lane -> 2 waves per SIMD, 264-512 -> 1, 136-168 -> 3, 104-128 -> 4
    assert [waves_per_simd(v, 0) for v in (256, 230, 176, 168, 257, 128, 64)] == [2, 2, 2, 3, 1, 4, 8]
    assert waves_per_simd(250, 8) == 1 and waves_per_simd(124, 8) == 3
