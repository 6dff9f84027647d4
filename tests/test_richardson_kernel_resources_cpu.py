"""Registers of the two Richardson kernels (KRichCombineCs, KRichMatchDs), without a GPU: neither may spill a VGPR or
use scratch.  The figures are the code-object metadata of the built library, read like
test_discspec_kernel_resources_cpu.py does; the test prints them."""
import pytest

from kernel_notes import kernel_resources

KERNELS = {
    "_Z12kernel_entryI14KRichCombineCsEvNT_6ParamsE": "KRichCombineCs",
    "_Z12kernel_entryI12KRichMatchDsEvNT_6ParamsE": "KRichMatchDs",
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
