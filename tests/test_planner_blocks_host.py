"""The layouts of the device-side control blocks (csrc/sogm_handover.hpp: FlowBlock of the dataflow replan, FlightBlock
of the flight, UpdateBlock of the update flow) on the host, no GPU: compiled with the host compiler (tests/planner_blocks_host_test.cpp).

Checked there, for 1, 2, 3, 127, 128, 129, 1000 and 65535 agents: the regions lie in offset order without gap or overlap and
end within words(A), and carve() hands out exactly those offsets; the replan zeroes [0, FLOW_HDR + 2A), fills
[FLOW_HDR + 2A, FLOW_HDR + 6A) with -1 and keeps its generation word at FLOW_HDR + 6A; the flight's rings hold the smallest
power of two >= 2A slots, its three 64-bit queues start on even words, and a call zeroes exactly the words in front of the
parked lists — the exchange's ready words among them, the urgent queue behind them; the offsets at 128 agents as literals.
For 1, 2 and 128 agents the update flow's block holds 2048 + 32 A words, and its ticket, its error word and every agent's
progress word lie on distinct 128-byte lines inside it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_control_block_layouts_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    exe = str(tmp_path / "planner_blocks_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "planner_blocks_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "planner blocks host ok" in out.stdout
