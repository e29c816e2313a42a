"""CPU: the role arithmetic of the scatter GEMM's tail split (csrc/nr_scatter_tail.h, the text the kernel and its launcher
compile) -- csrc/nr_scatter_tail_check.cpp built as a plain host program: for R = 256, nk in {1, 7, 38} and every tile count
0 .. 3R + 1 the roles cover each (tile, k-step) exactly once and never leave the grid."""
import os
import shutil
import subprocess

from newsrecommendation_amd import _lib


def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return [shutil.which(c)]
    hipcc = shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))      # the compiler the library itself is built with
    assert hipcc, "no C++ compiler found"
    return [hipcc, "-x", "c++"]


def test_tail_roles_cover_every_tile_and_k_step_once(tmp_path):
    exe = str(tmp_path / "nr_scatter_tail_check")
    src = os.path.join(_lib.CSRC_DIR, "nr_scatter_tail_check.cpp")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", _lib.CSRC_DIR, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "scatter tail roles ok" in r.stdout
