"""CPU: the velocity audit (include/sogm_abi.h "velocity audit") without a GPU.
  1. the body of csrc/sogm_velaudit.hpp, compiled with the host compiler (tests/velaudit_rules_host_test.cpp), against the numpy
     reading of the header (tests/velocity_audit_reference.py), field for field: hand-built rows on every comparison of the rule
     (tests/velocity_audit_fixtures.py), and the oracle's lists over the velocity fixture.  The same program under
     -fsanitize=address,undefined runs them clean;
  2. the hand-built rows are what they are named for;
  3. the oracle's velocity estimation over helpers.velocity_fixture_inputs() with the seeded truth arrays fills every class and
     bin (the GPU test tests/test_velocity_audit_gpu.py runs the same inputs: it cannot pass on an empty class);
  4. the entries: declared, exported, bound; their refusals; no device, said loudly."""
import ctypes as C
import functools
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import velocity_audit_fixtures as vfx  # noqa: E402
import velocity_audit_reference as vref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reading(c):
    return vref.audit_agent(c["born"], c["src"], len(c["truth"]), c["truth"], c["codes"],
                            dict(speed_tolerance=c["tol"], n_codes=c["n_codes"]), ok=c.get("ok", True),
                            range_len=c.get("range_len", len(c["truth"])), max_points=c.get("max_points", 64))


def line_of(c):
    return vfx.case_line(c["born"], c["src"], c["truth"], c["codes"], c["tol"], c["n_codes"], ok=c.get("ok", True),
                         range_len=c.get("range_len"), max_points=c.get("max_points", 64))


def want_of(row, table):
    return ["R " + " ".join(str(int(v)) for v in row), ("T " + " ".join(str(int(v)) for v in table.reshape(-1))).rstrip() if table is not None else "T"]


@functools.lru_cache(maxsize=None)
def oracle_lists():
    """per sequence of the velocity fixture: the oracle's new-born list after the last frame, its source index (recovered by
    exact position match against the list the same frames give with labels on the last one), the truth arrays"""
    pop = importlib.import_module("pred-occ-planner_amd")
    orc = importlib.import_module("oracle.binding")
    orc.lib()
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    spec = pop.config.make_spec("parity", map_kind=2)
    params, tabs = dsp.make_dsp_params(spec.T), dsp.make_tables(11, n_gauss=1 << 16, n_rand=1 << 12)
    out = []
    for index, s in enumerate(helpers.velocity_fixture_inputs()):
        n = len(s["frames"][-1]["points"])
        labels, codes = vfx.truth_arrays(index, n)
        est, given = orc.DspOracle(spec, params, tabs), orc.DspOracle(spec, params, tabs)
        for k, fr in enumerate(s["frames"]):
            last = k == len(s["frames"]) - 1
            assert est.update(fr["points"], None, fr["pos"], fr["quat"], fr["stamp"]) == 1
            assert given.update(fr["points"], labels if last else None, fr["pos"], fr["quat"], fr["stamp"]) == 1
        born, _ = est.born()
        ident, _ = given.born()
        est.close()
        given.close()
        assert ident.shape == (n, 7) and np.array_equal(ident[:, 3:].view(np.uint32), labels.view(np.uint32))
        where = {}
        for i, p in enumerate(ident[:, :3]):
            assert where.setdefault(p.tobytes(), i) == i, (s["branch"], "two input points share a position")
        src = np.array([where[p.tobytes()] for p in born[:, :3]], np.int64)
        assert len(np.unique(src)) == len(src), s["branch"]
        out.append(dict(branch=s["branch"], born=born, src=src, truth=labels, codes=codes, tol=vfx.TOLERANCE, n_codes=vfx.N_CODES,
                        max_points=5000))
    return out


def all_cases():
    return list(vfx.hand_built().values()) + oracle_lists()


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "velaudit_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "velaudit_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "velaudit")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "velaudit_san")
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    return out


@pytest.fixture(scope="module")
def expected():
    lines, want = [], []
    for c in all_cases():
        lines.append(line_of(c))
        want += want_of(*reading(c))
    return lines, want


def check_all(exe, tmp_path, expected):
    lines, want = expected
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    got = run.stdout.splitlines()
    assert len(got) == len(want) == 2 * len(lines)
    names = list(vfx.hand_built()) + [c["branch"] for c in oracle_lists()]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (names[i // 2], "row" if i % 2 == 0 else "per-code table", g, w)


def test_host_body_equals_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_body_runs_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


# ---- 2. the hand-built rows are what they are named for ---------------------------------------------------------------------
def test_the_ties_fall_as_the_header_says():
    hb = vfx.hand_built()
    row, tab = reading(hb["intensity and vx ties"])
    conf = row[4:12].reshape(2, 4)
    # rows 0, 2, 6: STATIC (0.01f itself, below it, NaN); 1, 4: TRACKED; 3, 5, 7: UNTRACKED (vx == -100, -10000, and a NaN vx:
    # "vx > -100" fails).  Truth: 1, 4, 5, 7 MOVING
    assert conf.tolist() == [[3, 0, 1, 0], [0, 2, 2, 0]] and row[3] == 0 and row[0] == row[1] == 8 and row[2] == 0
    assert tab.sum(axis=0)[:4].tolist() == [3, 2, 3, 0] and tab[3, 1] == 1 and tab[4, 2] == 3      # -1 -> ground; 3, -2, INT32_MIN -> other
    row, _ = reading(hb["speed ties"])
    # per T and truth class: e2 == T*T exactly (+T and -T) stays in the lower bin, one float above it moves up
    assert row[12:18].tolist() == [4, 6, 6, 6, 6, 2] and row[18:24].tolist() == [2, 3, 3, 3, 3, 1]
    row, _ = reading(hb["tolerance tie"])
    assert row[30] == 3 and row[4 + 4 + 1] == 4            # 0.25 exactly, 0.25 exactly (in y) and the exact estimate
    row, _ = reading(hb["tolerance zero"])
    assert row[30] == 1
    row, _ = reading(hb["direction ties"])
    # 14.9 deg and (2, 0) on (1, 0): 0;  45 deg exactly and 15.1 deg: 1;  one float past 45 deg: 2;  dot == 0 (twice) and
    # dot < 0: 3;  a zero estimate (and one of (0, -0)) on a moving truth: 4
    assert row[24:29].tolist() == [2, 2, 1, 3, 2], row[24:29].tolist()
    row, _ = reading(hb["nan inf clamp"])
    assert row[3] >= 4 and row[29] >= 3 * 10 ** 10 and row[17] >= 3      # three clamped errors at 1e4 m^2/s^2 each
    row, tab = reading(hb["codes"])
    # codes 0 and 2 have rows of their own (1 is not used), -1 is the ground's, and -2, n_codes, INT32_MIN and INT32_MAX share the last
    assert row[4:12].sum() == 14 and tab[:, :4].sum(axis=1).tolist() == [2, 0, 2, 2, 8] and tab[:, 3].sum() == 7
    row, tab = reading(hb["bad sources"])
    assert row[2] == vref.BAD_SOURCE and row[1] == 7 and row[4:12].sum() == 5 and row[4:12].reshape(2, 4)[:, 3].sum() == 2
    assert reading(hb["n_born zero"])[0][4:12].reshape(2, 4)[:, 3].tolist() == [2, 3]
    for name in ("n_in zero", "rejected update"):
        row, tab = reading(hb[name])
        assert row[2] == vref.SKIPPED and not np.delete(row, 2).any() and not tab.any()
    row, _ = reading(hb["clipped"])
    assert row[2] == vref.CLIPPED and row[0] == 4
    assert reading(hb["no codes"])[1] is None


# ---- 3. the oracle's lists fill every class ----------------------------------------------------------------------------------
def test_the_velocity_fixture_fills_every_class_and_bin():
    total = np.zeros(vref.ROW, np.int64)
    for c in oracle_lists():
        row, tab = reading(c)
        assert row[2] == 0 and row[4:12].sum() == row[0] == len(c["truth"]) and tab[:, :4].sum() == row[0], c["branch"]
        total += row
    print(total.tolist())
    assert (total[4:12] > 0).all(), total[4:12].tolist()
    assert (total[12:18] > 0).all() and (total[24:29] > 0).all(), (total[12:18].tolist(), total[24:29].tolist())
    assert (total[18:24] > 0).any() and total[3] > 0 and total[30] > 0 and total[29] > 0
    assert total[4 + 3] + total[8 + 3] > 0                      # DROPPED
    by = {c["branch"]: c for c in oracle_lists()}
    assert len(by["size_4_dropped_5_kept"]["born"]) == len(by["size_4_dropped_5_kept"]["truth"]) - 4
    assert len(by["cloud_1025"]["truth"]) == 1025 and len(by["cloud_2600"]["truth"]) == 2600


# ---- 4. the entries ----------------------------------------------------------------------------------------------------------
def good_prm(pop, **kw):
    p = pop._abi.SogmVelAuditParams()
    p.speed_tolerance, p.n_codes, p.flags = 0.25, 7, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PRM = [("n_codes", -1), ("n_codes", 1023), ("n_codes", 2 ** 31 - 1), ("speed_tolerance", -0.5), ("speed_tolerance", np.nan),
           ("speed_tolerance", np.inf), ("flags", 2), ("flags", -1)]


def test_the_entries_are_declared_exported_and_bound(pop):
    host = open(os.path.join(ROOT, "include", "sogm_abi.h")).read()
    debug = open(os.path.join(ROOT, "include", "sogm_abi_debug.h")).read()
    lib = C.CDLL(pop._abi.LIB_PATH)
    assert "int sogm_dsp_velocity_audit(" in host and "int sogm_dsp_download_born_source(" in debug
    for name in ("sogm_dsp_velocity_audit", "sogm_dsp_download_born_source"):
        assert hasattr(lib, name) and name in pop._abi.PROTOTYPES
    a = pop._abi
    assert C.sizeof(a.SogmVelAuditParams) == 16 and "/* 16 bytes */" in host and a.SOGM_VELAUDIT_ROW == 32
    assert "#define SOGM_VELAUDIT_ROW 32" in host
    assert [a.SOGM_VEL_STATIC, a.SOGM_VEL_TRACKED, a.SOGM_VEL_UNTRACKED, a.SOGM_VEL_DROPPED] == [0, 1, 2, 3]
    assert [a.SOGM_VELAUDIT_SKIPPED, a.SOGM_VELAUDIT_BAD_SOURCE, a.SOGM_VELAUDIT_CLIPPED, a.SOGM_VELAUDIT_ACCUMULATE] == [1, 2, 4, 1]
    assert [vref.STATIC, vref.TRACKED, vref.UNTRACKED, vref.DROPPED, vref.SKIPPED, vref.BAD_SOURCE, vref.CLIPPED] == [0, 1, 2, 3, 1, 2, 4]
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    assert all(hasattr(dsp.DspMap, m) for m in ("audit_velocity", "download_born_source")) and callable(dsp.velocity_scores)


def test_null_pointers_and_own_fields_are_refused_before_anything_else(pop):
    """with pointers that are never dereferenced: the refusals that need no handle come first"""
    lib, bad = pop.lib(), pop._abi.SOGM_ERR_INVALID_ARG
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    prm = good_prm(pop)
    for k in (0, 1, 3, 4, 5):
        args = [p, p, p, p, C.byref(prm), p, p, None]
        args[k] = None
        assert lib.sogm_dsp_velocity_audit(*args) == bad and b"sogm_dsp_velocity_audit: null pointer" in lib.sogm_last_error(), k
    assert lib.sogm_dsp_velocity_audit(p, p, None, p, C.byref(prm), p, p, None) == bad and b"truth_code" in lib.sogm_last_error()
    for field, v in BAD_PRM:
        assert lib.sogm_dsp_velocity_audit(p, p, p, p, C.byref(good_prm(pop, **{field: v})), p, p, None) == bad, (field, v)
        assert lib.sogm_last_error().startswith(b"sogm_dsp_velocity_audit: "), (field, v)
    assert lib.sogm_dsp_download_born_source(None, 0, None, 0, None) == bad


def test_without_a_gpu_the_entry_fails_loudly(pop):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = pop.lib()
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    for prm in (good_prm(pop), good_prm(pop, n_codes=1022, flags=1, speed_tolerance=0.0)):
        assert lib.sogm_dsp_velocity_audit(p, p, None, p, C.byref(prm), p, None, None) == pop._abi.SOGM_ERR_NO_DEVICE
        assert b"sogm_dsp_velocity_audit: no HIP device" in lib.sogm_last_error()


def test_velocity_scores():
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    row = np.zeros(32, np.int64)
    row[0], row[1] = 100, 90
    row[4:12] = [50, 5, 5, 6, 10, 12, 8, 4]                 # still: static tracked untracked dropped; moving: the same
    row[12:18] = [4, 2, 2, 1, 1, 0]                          # 10 scored of the 12 tracked (two NaN)
    row[3], row[29], row[30] = 2, 2_500_000, 6               # sum e2 = 2.5 -> rms 0.5
    s = dsp.velocity_scores(np.stack([row, np.zeros(32, np.int64)]))
    assert s["moving"] == 34 and s["still"] == 66 and s["detection_recall"] == 20 / 34 and s["detection_precision"] == 20 / 30
    assert s["tracked_share_of_moving"] == 12 / 34 and s["dropped_share"] == 0.1 and s["within_tolerance_share"] == 0.6
    assert abs(s["rms_error"] - 0.5) < 1e-12
    empty = dsp.velocity_scores(np.zeros(32, np.int64))
    assert empty["rms_error"] is None and empty["detection_precision"] is None and empty["dropped_share"] is None
