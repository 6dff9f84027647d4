"""Registers of the slow-discretization kernels (KSlowPrep, KSlowScatter, KSlowReduce, KSlowCombine: nft_nsev_slow.h), without a GPU.
One lane of the scatter kernel carries a 2x2 complex fp64 map through a loop of matrix exponentials; a spilled register
there is a round trip to HBM in every step.  None may spill a register or use scratch.  The figures are the code-object
metadata of the built library (spill counts and private segment size only), read with the ROCm LLVM tools like
test_discspec_kernel_resources_cpu.py does; the test prints the register counts."""
import pytest

from kernel_notes import kernel_resources

KERNELS = {
    "_Z12kernel_entryI9KSlowPrepEvNT_6ParamsE": "KSlowPrep",
    "_Z12kernel_entryI12KSlowScatterILi0ELb1EEEvNT_6ParamsE": "KSlowScatter<0, true>",
    "_Z12kernel_entryI12KSlowScatterILi0ELb0EEEvNT_6ParamsE": "KSlowScatter<0, false>",
    "_Z12kernel_entryI12KSlowScatterILi1ELb0EEEvNT_6ParamsE": "KSlowScatter<1, false>",
    "_Z12kernel_entryI12KSlowScatterILi2ELb0EEEvNT_6ParamsE": "KSlowScatter<2, false>",
    "_Z12kernel_entryI11KSlowReduceEvNT_6ParamsE": "KSlowReduce",
    "_Z12kernel_entryI12KSlowCombineEvNT_6ParamsE": "KSlowCombine",
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
