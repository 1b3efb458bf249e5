"""The resource owner (csrc/sogm_resources.hpp) on the host, no GPU: compiled with the host compiler and linked against a
counting stand-in for the HIP entry points it calls (tests/resources_host_test.cpp defines them; no GPU runtime is linked).

Checked there: after a scripted set-up of a dozen mixed acquisitions, two single releases and a regrow, releasing everything
leaves nothing live and releases every handle exactly once — streams first (each synchronised, then destroyed), then
events, then memory, in reverse order of acquisition within a kind; failing the k-th acquisition of a guarded set-up, for
every k, leaves the live counts where they were and every field of the set-up (its guard included) null, and a second
attempt succeeds; releasing a handle twice, a null handle or a handle held elsewhere is harmless."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resource_owner_against_a_counting_hip_stand_in(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if cxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("host compiler or HIP headers not available")
    exe = str(tmp_path / "resources_host_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "resources_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "resources host ok" in out.stdout
