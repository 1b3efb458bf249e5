"""CPU: the flight audit's C ABI on the host — host/sogm_facade.hpp's Audit wrapper compiles and links, refused arguments
give SOGM_ERR_INVALID_ARG, and without a GPU a well-formed call returns an error code instead of crashing."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_audit_facade_host(pop, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "audit_facade_host_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "audit_facade_host_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "audit facade host ok" in out.stdout


def test_audit_binding_refuses_bad_arguments(pop):
    abi, lib = pop._abi, pop.lib()
    prm = abi.SogmAuditParams()
    prm.body[:] = [0.4, 0.4, 0.45]
    prm.sample_dt, prm.goal_tolerance, prm.event_capacity = 0.01, 1.0, 0
    fake = C.c_void_p(0x1000)
    args = lambda period, n_local: (C.byref(prm), fake, 1, 4, None, 0.0, 0, period, 0, n_local, fake, fake, None, 0, fake,
                                    None, fake, None)
    assert lib.sogm_swarm_audit(*args(0.1, 5)) == abi.SOGM_ERR_INVALID_ARG
    assert lib.sogm_swarm_audit(*args(0.1001, 4)) == abi.SOGM_ERR_INVALID_ARG
    assert b"whole" in lib.sogm_last_error()
    assert C.sizeof(abi.SogmAuditAgent) == 104 and C.sizeof(abi.SogmAuditEvent) == 24 and C.sizeof(abi.SogmAuditParams) == 56
