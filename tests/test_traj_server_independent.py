"""The trajectory server's host body (csrc/sogm_trajserver.hpp: trajsrv_receive / trajsrv_timer, compiled with the host
compiler and -ffp-contract=off: tests/trajserver_rules_host_test.cpp, with a plain C++ evaluator) against the independent
reading of the reference's bezier_traj_server in tests/golden/traj_server_independent.json (written by
tests/golden/make_traj_server_fixture.py from the reference text, with a deque, a Bernstein-basis evaluation and its own
restatement of sogm_det::atan2).  Every case, named by its branch: sample times, traj_id, flags, the queue size after every
event and the overflow flag equal exactly; pos / vel / acc within 1e-12, yaw within 1e-9, yaw_dot within 2e-7
(traj_server_fixture.check).  The same program built with -fsanitize=address,undefined runs every case clean: the ring
indices are what that is for."""
import os
import shutil
import subprocess

import pytest

import traj_server_fixture as tsf

ROOT = tsf.ROOT


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "trajserver_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "trajserver_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "trajsrv")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "trajsrv_san")
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    return out


def case_text(case):
    p = case["prm"]
    lines = [f"P {p['replan_threshold']!r} {p['sample_dt']!r} {p['yaw_pi']!r} {p['yaw_dot_max']!r} {p['yaw_mode']}",
             f"I {case['t_trigger']!r} {case['init_yaw']!r} " + " ".join(repr(float(v)) for v in case["init_pos"]),
             f"T {case['t0']!r} {case['first_tick']} {case['period']!r} {case['receive_delay']!r} {len(case['ticks'])} "
             f"{case['m']}"]
    for t in case["ticks"]:
        if t["record"] is None or not t["received"]:
            lines.append("N")
            continue
        r = case["records"][t["record"]]
        nums = [r["time_start"]] + r["duration"] + [v for c in r["cpts"] for v in c]
        lines.append(f"R {len(r['duration'])} " + " ".join(repr(float(v)) for v in nums))
    return "\n".join(lines) + "\n"


def run_case(exe, case):
    run = subprocess.run([exe], input=case_text(case), capture_output=True, text=True)
    assert run.returncode == 0, (case["name"], run.returncode, run.stderr[-2000:])
    cmds, sizes, queue, final = [], [], [], None
    for line in run.stdout.splitlines():
        tag, *f = line.split()
        if tag == "C":
            cmds.append([float(v) for v in f[:13]] + [int(f[13]), int(f[14])])
            sizes.append(int(f[15]))
        elif tag == "E":
            sizes.append(int(f[0]))
        elif tag == "S":
            final = dict(zip(("ts", "te", "duration", "last_yaw", "last_yawdot"), map(float, f[:5])))
            final.update(zip(("size", "traj_id", "received", "overflow"), map(int, f[5:])))
        elif tag == "Q":
            queue.append([float(v) for v in f])
    return cmds, sizes, final, queue


@pytest.mark.parametrize("case", tsf.CASES, ids=[c["name"] for c in tsf.CASES])
def test_host_body_equals_the_independent_reading(exe, case):
    tsf.check(case, *run_case(exe, case))


def test_the_fixture_covers_every_branch():
    assert {"reset", "merge", "early", "early(k<0)", "silent", "held", "pop", "pop,tq<ts", "pop,t>duration"} <= set(
        tsf.FX["branches"])
    assert {"A.turn", "A.turn.wrap", "A.take", "B.turn", "B.turn.wrap", "B.take", "C.down", "C.up", "C.track",
            "C.hold"} <= set(tsf.FX["leaves"])
    ks = [b for c in tsf.CASES for b in c["branches"]]
    assert "merge k=118" in ks and "merge k=117" in ks and any(b.startswith("early(k<0)") for b in ks)
    assert {c["prm"]["replan_threshold"] for c in tsf.CASES} >= {0.02, 0.3, 0.5, 1.2}
    assert {(c["prm"]["yaw_mode"], c["prm"]["yaw_dot_max"]) for c in tsf.CASES} >= {(0, tsf.CASES[0]["prm"]["yaw_pi"]),
                                                                                   (1, 0.05)}
    assert any(c["final"]["overflow"] for c in tsf.CASES) and any(len(r["duration"]) == 16 for c in tsf.CASES
                                                                  for r in c["records"])


def test_host_body_runs_clean_under_the_sanitizers(exe_sanitized):
    for case in tsf.CASES:
        tsf.check(case, *run_case(exe_sanitized, case))
