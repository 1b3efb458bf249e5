"""The FSM rules the device kernels run (csrc/sogm_fsm.hpp: fsm_due / fsm_step) on the host, no GPU: compiled with the
host compiler (tests/fsm_rules_host_test.cpp; the header's device qualifiers sit behind __HIPCC__) and fed every tick of
the 24 agents of tests/golden/fsm_independent.json — the independent restatement of FiniteStateMachine::FSMCallback
(plan_manager/src/plan_manager.cpp:92-233).  State, failure counter, traj_start_time_ and the publication of all 2879
ticks must be equal, the doubles bit for bit (printed with 17 significant digits)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "fsm_independent.json")))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp("fsm_rules") / "fsm_rules_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fsm_rules_host_test.cpp"), "-o", out])
    return out


def test_fsm_rules_equal_the_independent_restatement(exe):
    n = 0
    for a, ticks in enumerate(FX["agents"]):
        text = "".join(f"{now!r} {ok} {safe} {reached}\n" for now, ok, safe, reached, *_ in ticks)
        run = subprocess.run([exe, repr(FX["traj_start0"]), repr(FX["replan_duration"]), repr(FX["replan_start_time"]),
                              str(FX["replan_max_failures"])], input=text, capture_output=True, text=True)
        assert run.returncode == 0, (a, run.returncode, run.stderr)
        lines = run.stdout.splitlines()
        assert len(lines) == len(ticks), (a, len(lines), len(ticks))
        for k, (line, (_, _, _, _, status, fails, ts, pub)) in enumerate(zip(lines, ticks)):
            got = line.split()
            assert got[0] == status and int(got[1]) == fails and float(got[2]) == ts, (a, k, line)
            if pub is None:
                assert got[3:] == ["none"], (a, k, line)
            elif pub[0] == "new":
                assert got[3:] == ["new"], (a, k, line)
            else:
                assert got[3] == "hover" and float(got[4]) == pub[1], (a, k, line)
            n += 1
    assert n == 2879
