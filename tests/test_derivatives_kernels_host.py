"""
CPU test of the kernels of csrc/deform_points_jet.hip (points_jet_kernel, points_jet_grad_prepare / _scatter, with
points_grad_clear / _finish of csrc/deform_points_grad.hip, which the program includes as well, at their two ends) as
host code under AddressSanitizer and UndefinedBehaviorSanitizer.  tests/cxx/points_jet_host_test.cpp is a
stand-alone program (its own main, no GPU, no HIP call, not loaded into Python): it compiles the kernels' device
functions as plain C++ against the stand-in runtime of tests/cxx/host_hip -- workgroups of one emulated thread, dynamic
LDS poisoned beyond the launch's size -- and runs 1, 2 and 3 axes, the two-point grid, grids read from global memory
and N = 1 on heap blocks of exactly the promised size; H is compared with a plain 4^n-tap evaluation in the program
itself, dP with step-1 differences of L, the rows with central differences, and two runs bit for bit.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clang():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for path in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(path):
            return path
    return None


def test_points_jet_kernels_as_host_code_under_sanitizers(tmp_path):
    clang = _clang()
    if clang is None:
        pytest.skip("the ROCm clang++ is not available")
    exe = str(tmp_path / "points_jet_host_test")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-x", "c++", "-I" + os.path.join(ROOT, "tests", "cxx", "host_hip"),
                    "-I" + os.path.join(ROOT, "elasticdeform_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "points_jet_host_test.cpp"), "-o", exe],
                   check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
