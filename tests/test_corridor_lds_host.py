"""The LDS layouts of the corridor translation unit (csrc/sogm_lp.hpp) on the host, no GPU: compiled with the host
compiler (tests/corridor_lds_host_test.cpp; the header's device-side parts sit behind __HIPCC__).

Checked there: the four byte totals as literals (LP wave 23868; segment 35900 and direct FIRI 37708 plus 8 bytes per 64
points, at capacities 1, 63, 64, 65, 4096, 16384; rules hook 26012); in every layout the regions lie in offset order
without gap or overlap, end at bytes(), and every double region starts on 8 bytes; the small state's fields fill its block;
the LP view a wave uses between two segments lies wholly in the head of the L-BFGS history; segment and direct-FIRI
layouts at 16384 points stay within 40960 bytes (four workgroups per compute unit)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_corridor_lds_layouts_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / "corridor_lds_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "corridor_lds_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "corridor lds host ok" in out.stdout
