"""CPU: the Cholesky and Jacobi routines of sgx_grm_pca (host_pca.h) as a stand-alone host program against closed-form
matrices, under the host sanitizers (tests/pca_check.cpp)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cholesky_and_jacobi_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "pca_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "saigegds_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pca_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "checks OK" in res.stdout
