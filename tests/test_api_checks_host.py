"""
CPU test of the argument checks the C entry points share (csrc/edhip_api.hip: check_naxis, check_displacement,
check_pairs, deformed_lengths, sample, fill_geometry, and the helpers of the strided-batch calls on the prefiltered grid:
check_batch_call ... batch_array), driven by a host-only C++ program on hostile descriptors -- rank 0 and 9, negative
extents, 0 and 8 deformed axes, null pointers where the ABI allows them.  No GPU, no HIP call.  The
program is tests/cxx/api_checks_test.cpp; its arrays are heap blocks of exactly the promised size, so the same build
with ``-Xarch_host -fsanitize=address,undefined`` added turns any read beyond them into a report.
"""
import os
import shutil
import subprocess

import pytest

from elasticdeform_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libedhip.so not built (run __graft_entry__.build())")
def test_shared_checks_on_hostile_descriptors(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "elasticdeform_amd", "csrc")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "api_checks_test")
    # (the program includes edhip_api.hip, which names the launchers of the other files: they come from the library)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "api_checks_test.cpp"),
                    "-L" + libdir, "-ledhip", "-Wl,-rpath," + libdir, "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
