"""The QP solver's memory plan (csrc/sogm_qp_layout.hpp) on the host, no GPU: compiled with the host compiler
(tests/qp_layout_host_test.cpp).  It checks the layout's offsets; the kernel computes its own pointers and is held to the
layout through the path it reports (tests/test_qp_gpu.py) and through the shared byte totals.

Checked there: for each of the four (fast, rows_in_lds) combinations the regions — blocks or band, the hot and the cold row
arrays (their sizes written out a second time from the twenty arrays), the 64-byte tail, K1 — lie in offset order in dynamic
LDS and in the agent's scratch without gap or overlap, doubles on 8 bytes and ints on 4, within the dynamic LDS granted and
the per-agent scratch stride; the check's
staging area lies inside the block area and ends at or before the hot rows; G, S, the hot and cold byte totals, the rows'
offset and K1's size for seven shapes as the solver's formulas gave them before they had one description, and the two
scratch sizes (471 552 and 17 280 bytes); the path of the six shapes of test_qp_gpu.py at 145 408, 147 456 and 149 504
bytes of dynamic LDS; every term of `fast` on both sides of its edge (8 | 9 pieces, 256 | 257 general rows, 1024 | 1025
safety rows, the staging bound at equality, blocks + hot rows == the grant | one byte less)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qp_layout_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / "qp_layout_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "qp_layout_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "qp layout host ok" in out.stdout


def test_qp_stat_slots_of_the_binding_match_the_header(pop):
    import re
    txt = open(os.path.join(ROOT, "include", "sogm_abi_debug.h")).read()
    slots = {name: int(val) for name, val in re.findall(r"\bSOGM_(QP_STAT_\w+) = (\d+)", txt)}
    assert len(slots) == 16 and slots["QP_STAT_PATH"] == 7 and slots["QP_STAT_N"] == 16
    mine = {k: v for k, v in vars(pop._abi).items() if k.startswith("QP_STAT_")}
    assert mine == slots
