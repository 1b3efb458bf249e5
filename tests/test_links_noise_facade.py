"""The C++ facade's message noise and belief audit (host/sogm_facade.hpp: Links::setNoise / sent / sentShift / auditBelief /
belief): tests/links_noise_facade_test.cpp compiles against them; without a GPU it checks the defaults and the refusals,
with one it sends a table through zero noise and through a localisation bias and audits the receivers' beliefs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_noise_and_belief_compile_and_run(pop, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    pop.lib()
    exe = str(tmp_path / "links_noise_facade_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "links_noise_facade_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "links noise facade ok" in out.stdout
