"""The arithmetic of the device-side hand-overs (csrc/sogm_handover.hpp) on the host, no GPU: compiled with the host
compiler (tests/handover_host_test.cpp; the header's device-side parts sit behind __HIPCC__).

Checked there: a ring tag decodes to its agent and matches the generation of its own position only (ring sizes 2, 4, 256,
every position up to 4 R, agents 0, 1, 65535), the zero word of a reset matches nothing, and the last position of the
longest flight of 65535 agents still has a positive tag; the same for the work queues' 64-bit tags at the positions where
the generation turns and at 2^32 - 1; descriptors round-trip for every kind, and the consecutive descriptors of one push
never reach the kind field; the failure codes have the values they had as bare literals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handover_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / "handover_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "handover_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "handover host ok" in out.stdout
