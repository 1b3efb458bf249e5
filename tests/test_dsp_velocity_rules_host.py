"""The single-lane rules of the velocity estimation (csrc/sogm_dsp_velocity.hpp) on the host, no GPU: compiled with the
host compiler (tests/dsp_velocity_rules_host_test.cpp), once plain and once as a stand-alone program under
-fsanitize=address,undefined.

Checked there: vel::std_sort against libstdc++'s std::sort with the same comparator — the id sequences equal, i.e. the order
of ties under that unstable sort — for n = 0, 1, 2, 15, 16, 17, 33, 100, 256 with all sizes equal, seeded sizes with many
ties, and strictly decreasing sizes, and vel::heap_sort against std::partial_sort(f, f + n, f + n); the assignment against
brute force over all injections on cost matrices of distinct powers of two (unique optimum, every sum exact in fp32) for
(R, C) = (1,1), (1,4), (4,1), (2,3), (3,4), (4,3), (4,4), three seeds each, the transposed view included; every gate closed: no
match, velocities stay -10000 / 0.55; a matched pair faster than maximum_velocity: zero velocity, counted as matched; the
possibly-dynamic split of six clusters of the four kinds, two of them on the bounds (size 200, centre height 1.5), with
dynseq, offsets, total_dyn and n_static as literals; the dynamic-LDS layout for max_pts = 1, 16, 7400, 8192: the five arrays
disjoint, in order, ending at bytes(max_pts) = 20 max_pts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dsp_velocity_rules_host_test"


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
    assert "dsp velocity rules host ok" in out.stdout


def test_velocity_rules_on_the_host(tmp_path):
    cmd, exe = _compile(tmp_path, [])
    subprocess.check_call(cmd)
    _run(exe)


def test_velocity_rules_on_the_host_under_the_sanitizers(tmp_path):
    cmd, exe = _compile(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    _run(exe)
