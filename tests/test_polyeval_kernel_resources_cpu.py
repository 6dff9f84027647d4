"""Registers of the polynomial evaluation kernels (KPolyEval<false>, KPolyEval<true>, KPolyJoin: nft_kernels.h), without
a GPU.  One lane of KPolyEval carries 8 complex Horner chains (16 with the derivative) through a loop over the whole
polynomial; a spilled register there is a round trip to HBM in every step.  None may spill a register or use scratch.
The figures are the code-object metadata of the built library, read like test_nsev_slow_kernel_resources_cpu.py does;
the test prints the register counts."""
import pytest

from kernel_notes import kernel_resources

KERNELS = {
    "_Z12kernel_entryI9KPolyEvalILb0EEEvNT_6ParamsE": "KPolyEval<false>",
    "_Z12kernel_entryI9KPolyEvalILb1EEEvNT_6ParamsE": "KPolyEval<true>",
    "_Z12kernel_entryI9KPolyJoinEvNT_6ParamsE": "KPolyJoin",
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
