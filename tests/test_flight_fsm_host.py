"""No GPU: the host side of the flight under the FSM (sogm_planner_set_flight_fsm).  The binding's SogmFlightFsm against
the header's layout, the ABI number, and the per-agent bodies that the stand-alone FSM kernels and the flight share
(csrc/sogm_fsm.hpp: fsm_inputs_agent, fsm_hover_record) compiled with the host compiler (tests/flight_fsm_host_test.cpp)
and flown through every tick of the 24 agents of tests/golden/fsm_independent.json — the independent restatement of
FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233): who is due and from when follows from the
fixture's previous state, state / failure counter / traj_start_time_ / publication are the fixture's, and a hover record
starts at the fixture's hover start, at the agent's position."""
import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "fsm_independent.json")))
CODE = {"NEW_PLAN": 0, "EXEC_TRAJ": 1, "REPLAN": 2, "GOAL_REACHED": 3}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp("flight_fsm") / "flight_fsm_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "flight_fsm_host_test.cpp"), "-o", out])
    return out


def test_binding_struct_matches_the_header(exe):
    abi = importlib.import_module("pred-occ-planner_amd._abi")
    got = [int(v) for v in subprocess.run([exe, "layout"], capture_output=True, text=True, check=True).stdout.split()]
    S = abi.SogmFlightFsm
    names = ("prm", "check_duration", "state_inout", "log_state", "log_due", "log_safe", "log_reached", "log_pub",
             "log_hover_start", "log_own")
    assert [f[0] for f in S._fields_] == list(names)
    assert got[0] == ctypes.sizeof(S) == 112
    assert got[1:11] == [getattr(S, n).offset for n in names]
    assert got[11] == abi.SOGM_ABI_VERSION == 6
    assert "sogm_planner_set_flight_fsm" in abi.PROTOTYPES


def test_header_still_says_abi_6_and_names_the_entry():
    text = open(os.path.join(ROOT, "include", "sogm_abi.h")).read()
    assert re.search(r"^#define SOGM_ABI_VERSION 6$", text, re.M)
    assert "int sogm_planner_set_flight_fsm(sogm_planner *p, const SogmFlightFsm *fsm_or_null);" in text
    assert "sogm_flight_run ignores the mask" not in text


def test_shared_bodies_equal_the_independent_restatement(exe):
    n = hovers = 0
    for a, ticks in enumerate(FX["agents"]):
        text = "".join(f"{now!r} {ok} {safe} {reached}\n" for now, ok, safe, reached, *_ in ticks)
        run = subprocess.run([exe, repr(FX["traj_start0"]), repr(FX["replan_duration"]), repr(FX["replan_start_time"]),
                              str(FX["replan_max_failures"])], input=text, capture_output=True, text=True)
        assert run.returncode == 0, (a, run.returncode, run.stderr)
        lines = run.stdout.splitlines()
        assert len(lines) == len(ticks), (a, len(lines), len(ticks))
        prev = (CODE["NEW_PLAN"], FX["traj_start0"])
        rec = (0, 0.0)   # n_pieces, time_start of the record the agent executes
        for k, (line, (now, _, _, reached, status, fails, ts, pub)) in enumerate(zip(lines, ticks)):
            head, mid, tail = (part.split() for part in line.split("|"))
            want_due = (1 if prev[0] == 0 and (now - prev[1]) > 1.0 else 0) | (2 if prev[0] == 2 else 0)
            want_t = now + FX["replan_start_time"] if prev[0] == 2 else now
            assert int(head[0]) == want_due and float(head[1]) == want_t and int(head[2]) == reached, (a, k, line)
            assert mid[0] == status and int(mid[1]) == fails and float(mid[2]) == ts, (a, k, line)
            if pub is None:
                assert mid[3:] == ["none"] and (int(tail[0]), float(tail[1])) == rec, (a, k, line)
            elif pub[0] == "new":
                assert mid[3:] == ["new"] and int(tail[0]) == 1 and float(tail[1]) == want_t, (a, k, line)
            else:
                assert mid[3] == "hover" and float(mid[4]) == pub[1], (a, k, line)
                assert int(tail[0]) == 1 and float(tail[1]) == pub[1], (a, k, line)
                hovers += 1
            rec = (int(tail[0]), float(tail[1]))
            prev = (CODE[status], ts)
            n += 1
    assert n == 2879 and hovers > 0
