"""Registers of the kernels of the guess-free batched discrete spectrum (group "discroots": KDsGather, KAberthB*,
KDsCandidates), without a GPU.  The Newton kernel runs 8 Horner chains with derivative and error chains per lane --
what it keeps in registers it reads in every step of an O(n^2) loop -- so none may spill a VGPR or use scratch, and
the LDS of each lets two workgroups share a CU.  The figures are the code-object metadata of the built library, read
with the ROCm LLVM tools like test_discspec_kernel_resources_cpu.py does; the test prints them."""
import pytest

from kernel_notes import kernel_resources

KERNELS = {
    "_Z12kernel_entryI9KDsGatherEvNT_6ParamsE": "KDsGather",
    "_Z12kernel_entryI13KAberthBStartEvNT_6ParamsE": "KAberthBStart",
    "_Z12kernel_entryI14KAberthBNewtonEvNT_6ParamsE": "KAberthBNewton",
    "_Z12kernel_entryI11KAberthBSumEvNT_6ParamsE": "KAberthBSum",
    "_Z12kernel_entryI13KAberthBApplyEvNT_6ParamsE": "KAberthBApply",
    "_Z12kernel_entryI12KAberthBStepEvNT_6ParamsE": "KAberthBStep",
    "_Z12kernel_entryI13KDsCandidatesEvNT_6ParamsE": "KDsCandidates",
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
    # 256 lanes = 4 waves, one per SIMD: two workgroups per CU need at most 256 VGPRs per lane and half the LDS
    assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256, (kernel, r)
