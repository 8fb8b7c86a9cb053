"""The ownership helpers of qdrant_amd/csrc/dev_mem.hpp (DevBuf, Staging, dev_upload) on the host: tools/dev_mem_check.cpp is built with the host
compiler against a fake HIP allocator and run.  It fails every allocation and copy of functions written the way the one-shot entry points are, and
checks that nothing stays live and nothing is freed twice.  No GPU and no HIP runtime are needed; the HIP headers are."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_dev_mem_check(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dev_mem_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "qdrant_amd", "csrc"),
         os.path.join(ROOT, "tools", "dev_mem_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout
