"""The flight's compute-unit partition (csrc/sogm_flight_layout.hpp) on the host, no GPU: compiled with the host compiler
(tests/flight_layout_host_test.cpp).

Checked there: flight_unit_of puts 16 of 256 compute units into each of the 16 units; six configurations' grids and resident
units as literals (whole device, two engines at either end, a reserved unit, a rest that is cut); QP, search and map hold
the same number of units in every shader engine they touch, the rest does unless it is cut; at 256 compute units the four
masks hold 16 compute units per unit, are disjoint and cover the device together with the reserved units, and the launches
are sized by what is resident ({2,1,7,6}: 32, 16, 96, 96 compute units); {5,2,5,4} is refused as unplaceable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flight_partition_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / "flight_layout_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "flight_layout_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "flight layout host ok" in out.stdout
