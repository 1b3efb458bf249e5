"""What the particle map is made of (csrc/sogm_dsp.hpp) on the host, no GPU: compiled with the host compiler
(tests/dsp_rules_host_test.cpp), once plain and once as a stand-alone program under -fsanitize=address,undefined.

Checked there: keep_smallest, the sorted bounded insertion of the ordered first-fit, against "sort everything, take the first
cap" for cap 1, 2, 16 and 20 over streams of 0 to 3 cap distinct keys in ascending, descending and seeded order, with and
without the id array; lowest_free for every occupancy of a 4-slot voxel and, for 16 slots, with none, one and all taken; the
buffer table for (A, V, NP, max_pts, nb) = (1, 8, 4, 16, 2) and (3, 1000, 60, 64, 20), DspDev filled by the function
sogm_dsp_create uses: every accessor's base of agent a is a times the table's per-agent count of each array it addresses,
the last agent's part ends at the allocated total, and no array of the table is without an accessor."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dsp_rules_host_test"


def _compile(tmp_path, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / NAME)
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"), os.path.join(ROOT, "tests", NAME + ".cpp"), "-o", exe]
    return cmd, exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert "dsp rules host ok" in out.stdout


def test_first_fit_rules_and_buffer_table_on_the_host(tmp_path):
    cmd, exe = _compile(tmp_path, [])
    subprocess.check_call(cmd)
    _run(exe)


def test_first_fit_rules_and_buffer_table_on_the_host_under_the_sanitizers(tmp_path):
    cmd, exe = _compile(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    _run(exe)
