"""The host-readable headers of the HNSW walk, checked without a GPU: tools/hnsw_walk_plan_check.cpp sweeps the launch decisions of
qdrant_amd/csrc/hnsw_walk_plan.hpp (what a search stages, its visited set, the PQ image, the capacities, the slots, the refusals) against the sequence of
assignments they replaced, written out longhand; tools/hnsw_layout_check.cpp sweeps the LDS layout of qdrant_amd/csrc/hnsw_layout.hpp.  Both are built
with the host compiler and run; neither needs HIP."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["hnsw_walk_plan_check", "hnsw_layout_check"])
def test_hnsw_host_check(tmp_path, name):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1","-I" + os.path.join(ROOT, "qdrant_amd", "csrc"), os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith(name) and re.search(r"\b[1-9][0-9]* combinations\b", last), run.stdout
    assert re.search(r"\bok\b", last), run.stdout
