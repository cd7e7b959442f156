"""The table layout of the set-test, conditional and Firth entries (saigegds_amd/csrc/host_tabs.h) on its own:
tests/tab_layout_check.cpp, a stand-alone host program, is built with the host compiler under
-fsanitize=address,undefined and run.  It lays out every list of three slots over element sizes 1, 4, 8 and
sizeof(SkatTile) and counts 0, 1, 15, 16, 17, asserts alignment, order, bounds and the cost of an empty slot, and
writes and reads every element in a heap buffer of exactly bytes() bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tab_layout_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tab_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "saigegds_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tab_layout_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "8000 slot lists OK" in res.stdout
