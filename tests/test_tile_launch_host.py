"""
CPU test of the tile launcher's host arithmetic (csrc/ed_tile_host.h): the scratch layout -- regions aligned, in order,
disjoint, byte for byte the sums the launcher and deform_tile_workspace_bytes used to carry separately, and the
reservation never smaller than what a launch asks for --, the one decision on how a control grid of a given width is
served (both sides of every threshold, against the logic deform_tile_supported and the launcher used to hold in
copies), the addressing limits and the strip lengths.  Driven by a host-only C++ program, tests/cxx/tile_launch_host_test.cpp,
which includes the header alone (no kernel is compiled) and links the built library for k1z_r_bytes and
deform_tile_workspace_bytes.  No GPU, no HIP call.
"""
import os
import shutil
import subprocess

import pytest

from elasticdeform_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libedhip.so not built (run __graft_entry__.build())")
def test_layout_wide_decision_limits_and_strips(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "elasticdeform_amd", "csrc")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "tile_launch_host_test")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-x", "hip", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "tile_launch_host_test.cpp"),
                    "-L" + libdir, "-ledhip", "-Wl,-rpath," + libdir, "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
