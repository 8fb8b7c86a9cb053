"""The tile walk of the prefilter scans over a derived copy (qdrant_amd/csrc/split_tiles.hpp) on the host: tools/split_tiles_check.cpp is built with the
host compiler and run.  For every sample stride 2..255 and every tile count 0..69, around the stride and its double, 1 000 and 39 063 (the headline's),
it checks that the strided launch and its complement together visit every tile exactly once, that the unphased launch is the identity, that the blocks
of any grid 1..300 share out exactly the launch's tiles, and that the launchers' grid never exceeds the CUs or the tiles and is empty for no rows.
No GPU and no HIP runtime are needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_tiles_check(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "split_tiles_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "qdrant_amd", "csrc"), os.path.join(ROOT, "tools", "split_tiles_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout
