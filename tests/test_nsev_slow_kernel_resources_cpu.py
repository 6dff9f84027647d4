"""Registers of the slow-discretization kernels (KSlowPrep, KSlowScatter, KSlowReduce, KSlowCombine: nft_nsev_slow.h), without a GPU.
One lane of the scatter kernel carries a 2x2 complex fp64 map through a loop of matrix exponentials; a spilled register
there is a round trip to HBM in every step.  None may spill a register or use scratch.  The figures are the code-object
metadata of the built library (spill counts and private segment size only), read with the ROCm LLVM tools like
test_discspec_kernel_resources_cpu.py does; the test prints the register counts."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fnft_amd", "lib", "libfnft_amd.so")
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


def _tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    path = shutil.which(name)
    assert path, "%s (ROCm LLVM tools) not found" % name
    return path


@pytest.fixture(scope="module")
def resources():
    from fnft_amd import build
    build.build()
    found = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(LIB, os.path.join(d, "lib.so"))
        subprocess.run([_tool("llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        objs = sorted(f for f in os.listdir(d) if "gfx950" in f)
        assert objs, "no gfx950 code object in the library"
        for co in objs:
            notes = subprocess.run([_tool("llvm-readelf"), "--notes", os.path.join(d, co)], check=True,
                                   stdout=subprocess.PIPE, text=True).stdout
            cur = {}
            for line in notes.splitlines():   # one record per kernel, opened by .agpr_count, named by .symbol
                m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip()
                if k == "agpr_count":
                    cur = {}
                if k in KEYS and k not in cur:
                    cur[k] = int(v)
                elif k == "symbol" and v.endswith(".kd") and v[:-3] in KERNELS:
                    found[KERNELS[v[:-3]]] = cur
    return found


@pytest.mark.parametrize("kernel", sorted(KERNELS.values()))
def test_no_spill_no_scratch(resources, kernel):
    r = resources.get(kernel)
    assert r is not None and all(k in r for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")), \
        (kernel, r)
    print(kernel, r)
    assert r["vgpr_spill_count"] == 0, (kernel, r)
    assert r["private_segment_fixed_size"] == 0, (kernel, r)
