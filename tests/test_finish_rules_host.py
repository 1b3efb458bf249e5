"""The rule "where did this replan end" (csrc/sogm_finish.hpp) on the host, no GPU: compiled with the host compiler
(tests/finish_rules_host_test.cpp; the header's device bodies sit behind __HIPCC__).

Checked there: replan_outcome against a table written out by hand — every combination of ret in {0, 1, 3}, npoly in
{-1, 0, 1, 16}, status in {-100, -7, 0, 1, 2, 3} and safe in {false, true}, 144 in all, the expected SOGM_CNT_* index as a
literal 0-4 (precedence: no path, no corridor, QP not solved, unsafe, else ok); the form the device bodies call gives the
same index and reads the QP's status only behind a search and corridors; "solved" is the outcome with safe = true being ok
and "good" the outcome being ok."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replan_outcome_rule_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / "finish_rules_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "finish_rules_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "finish rules host ok" in out.stdout
