"""The grid pool's bookkeeping (csrc/sogm_gridpool.hpp) on the host, no GPU: compiled with the host compiler against
nothing but the HIP headers' handle types (tests/gridpool_host_test.cpp; the header calls no HIP entry point).

Checked there, with the invariants after every step ({current} + ready + dirty is a partition of the slots; with two grids
or more, precleared <=> ready is not empty): adoption is FIFO over 10 ticks with 2 and with 3 grids; a rebuild from every
current slot to every size, acquisition succeeding or failing, keeps the current grid's pointer, logs, event, tracked flag
and history counters together in slot 0 and leaves ready empty, dirty = every spare, the spares untracked with zeroed
history (a failed acquisition: the old pool); a dense writer untracks only the current slot; the pre-stamp target is
adoptable only while it is the front of ready, and a plain update gets it back as stale."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_pool_bookkeeping_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if cxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("host compiler or HIP headers not available")
    exe = str(tmp_path / "gridpool_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "gridpool_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "gridpool host ok" in out.stdout
