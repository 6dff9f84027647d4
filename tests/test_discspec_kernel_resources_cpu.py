"""Registers of the batched discrete-spectrum kernels (KDsBox, KDsNewton, KDsFilter, KDsNorm) and of the chunk-parallel
scatterer (KBs*), without a GPU: fp64 2x2
complex products with derivative maps are register-heavy, and a spilled register is a round trip to HBM inside every
Newton iteration.  None may spill a VGPR or use scratch.  The figures are the code-object metadata of the built
library, read with the ROCm LLVM tools like test_kernel_resources_cpu.py does; the test prints them."""
import pytest

from kernel_notes import kernel_resources

KERNELS = {
    "_Z12kernel_entryI6KDsBoxEvNT_6ParamsE": "KDsBox",
    "_Z12kernel_entryI9KDsNewtonILb0EEEvNT_6ParamsE": "KDsNewton<false>",
    "_Z12kernel_entryI9KDsNewtonILb1EEEvNT_6ParamsE": "KDsNewton<true>",
    "_Z12kernel_entryI9KDsFilterEvNT_6ParamsE": "KDsFilter",
    "_Z12kernel_entryI7KDsNormILb0EEEvNT_6ParamsE": "KDsNorm<false>",
    "_Z12kernel_entryI7KDsNormILb1EEEvNT_6ParamsE": "KDsNorm<true>",
    # the chunk-parallel scatterer the batched kernels share their 2x2 map arithmetic with
    "_Z12kernel_entryI8KBsChunkILb0EEEvNT_6ParamsE": "KBsChunk<false>",
    "_Z12kernel_entryI8KBsChunkILb1EEEvNT_6ParamsE": "KBsChunk<true>",
    "_Z12kernel_entryI10KBsCombineILb0EEEvNT_6ParamsE": "KBsCombine<false>",
    "_Z12kernel_entryI10KBsCombineILb1EEEvNT_6ParamsE": "KBsCombine<true>",
    "_Z12kernel_entryI9KBsMatrixEvNT_6ParamsE": "KBsMatrix",
    "_Z12kernel_entryI6KBsPhiEvNT_6ParamsE": "KBsPhi",
    "_Z12kernel_entryI6KBsPsiEvNT_6ParamsE": "KBsPsi",
    "_Z12kernel_entryI9KBsMetricEvNT_6ParamsE": "KBsMetric",
    "_Z12kernel_entryI7KBsPickEvNT_6ParamsE": "KBsPick",
}
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


@pytest.fixture(scope="module")
def resources():
    from fnft_amd import build
    build.build()
    return kernel_resources(KERNELS, KEYS)


@pytest.mark.parametrize("kernel", sorted(KERNELS.values()))
def test_no_spill_no_scratch(resources, kernel):
    r = resources.get(kernel)
    assert r is not None and all(k in r for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")), \
        (kernel, r)
    print(kernel, r)
    assert r["vgpr_spill_count"] == 0, (kernel, r)
    assert r["private_segment_fixed_size"] == 0, (kernel, r)
