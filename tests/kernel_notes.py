"""Shared by the kernel-resource tests (test_kernel_resources_cpu.py, test_discspec_kernel_resources_cpu.py,
test_nsev_slow_kernel_resources_cpu.py): the ROCm LLVM tools, the gfx950 code objects of the built library and the
per-kernel records of their metadata notes.  No GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fnft_amd", "lib", "libfnft_amd.so")


def tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    path = shutil.which(name)
    assert path, "%s (ROCm LLVM tools) not found" % name
    return path


def kernel_resources(kernels, keys, lib=LIB):
    """{kernels[symbol]: {key: int}} for every kernel_entry<K> symbol of `kernels` found in the library's gfx950 code
    objects (one per translation unit), with those of `keys` its metadata record holds."""
    found = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([tool("llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        objs = sorted(f for f in os.listdir(d) if "gfx950" in f)
        assert objs, "no gfx950 code object in the library"
        for co in objs:
            notes = subprocess.run([tool("llvm-readelf"), "--notes", os.path.join(d, co)], check=True,
                                   stdout=subprocess.PIPE, text=True).stdout
            # one metadata record per kernel, opened by its first key (.agpr_count); .symbol names it (the argument
            # records inside it have a .name but no .symbol)
            cur = {}
            for line in notes.splitlines():
                m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip()
                if k == "agpr_count":
                    cur = {}
                if k in keys and k not in cur:
                    cur[k] = int(v)
                elif k == "symbol" and v.endswith(".kd") and v[:-3] in kernels:
                    found[kernels[v[:-3]]] = cur
    return found
