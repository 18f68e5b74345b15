"""CPU: the LDS layout of the resident-image form of the split-operand lone-tile GEMM (csrc/gemm_x3_halo.h) is plain integer arithmetic,
shared by the kernel and its host-side predicate.  tools/host/gemm_x3_halo_check.cpp replays the staging and every fragment read of
the 64 pixels x 9 taps on a host array of the image's size -- every halo pixel index in [0, 100), tap (r, s) reads the image shifted
by (r - 1, s - 1) with zeros outside, every ds_read_b128 lane group on 16 different slots, Ci = 128 fits the LDS and nothing larger
does -- and is built and run here as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_halo_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_x3_halo_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "self-diagnosing-gan_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host", "gemm_x3_halo_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
