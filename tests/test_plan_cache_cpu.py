"""The per-device host state of the shim (fnft_amd/csrc/nft_plan_cache.h: the bounded plan cache and the device registry)
as a stand-alone program on fake handles, tests/host/plan_cache_main.cpp: one thread is inside a call on device 0 while
another takes device 1 past the cache's capacity, and no handle may be destroyed while its call uses it.  Built and run
three ways: plain, under ThreadSanitizer and under AddressSanitizer + UBSan.  No GPU, no HIP, nothing loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "plan_cache_main.cpp")
HEADER = os.path.join(HERE, "..", "fnft_amd", "csrc", "nft_plan_cache.h")
BASE = ["g++", "-std=c++20", "-pthread", "-O1", "-g"]
VARIANTS = {"plain": [], "tsan": ["-fsanitize=thread"], "asan_ubsan": ["-fsanitize=address,undefined"]}


def _links(flags, tmp_path):
    """Does a one-line program link with these flags (is the sanitizer's runtime installed)?"""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    return subprocess.run(BASE + flags + [str(one), "-o", str(tmp_path / "one")], capture_output=True).returncode == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_plan_cache_program(variant, tmp_path):
    assert shutil.which("g++"), "g++ is needed to build tests/host/plan_cache_main.cpp"
    assert os.path.exists(HEADER)
    flags = VARIANTS[variant]
    if flags and not _links(flags, tmp_path):
        pytest.skip("g++ cannot link a one-line program with " + " ".join(flags))
    exe = tmp_path / ("plan_cache_" + variant)
    b = subprocess.run(BASE + flags + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "plan_cache_main: ok" in r.stdout
    for word in ("Sanitizer", "runtime error", "WARNING", "ERROR"):
        assert word not in r.stderr, r.stderr
