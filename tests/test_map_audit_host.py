"""CPU: the map audit (include/sogm_abi.h "map audit") without a GPU.
  1. the bodies of csrc/sogm_mapaudit.hpp, compiled with the host compiler (tests/mapaudit_rules_host_test.cpp), against the
     numpy reading of the header (tests/map_audit_reference.py), bit for bit: word dilation at L = 1, 63, 64, 65, 66, 128, 130
     for r = 0 .. 3 with bits at 0, 63, 64 and L - 1; the occupancy test; the frustum test with exact ties; the layout's sizes.
     The same program under -fsanitize=address,undefined runs them clean;
  2. the reading against a different algorithm: pairwise Chebyshev distances on random grids;
  3. the entry: declared, exported, bound; null pointers and prm's own fields refused; no device, said loudly."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_audit_reference as mref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = np.float32(0.15)


def h64(v):
    return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(v, np.float64).reshape(-1).view(np.uint64))


def h32(v):
    return " ".join(f"{int(b):08x}" for b in np.ascontiguousarray(v, np.float32).reshape(-1).view(np.uint32))


def words_of(xs, L):
    w = [0] * mref.row_words(L)
    for x in xs:
        w[x // 64] |= 1 << (x % 64)
    return w


# camera z along world +x, camera x along world +y, camera y along world +z (a proper rotation: a cyclic permutation)
PERM = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64).reshape(9)
c, s = np.cos(0.37), np.sin(0.37)
GENERIC = (np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(-0.21), -np.sin(-0.21)],
                                                                     [0, np.sin(-0.21), np.cos(-0.21)]]) @ PERM.reshape(3, 3)).reshape(9)


def frustum_cases():
    """(rot, near, far, tan_h, tan_v, dims, cells [n, 3]) — with PERM q_z = p_0, q_x = p_1, q_y = p_2"""
    dims = (20, 20, 20)
    px = mref.centres(dims, RES)[0]
    grid = np.array([(x, y, z) for x in range(8, 20) for y in range(0, 20, 3) for z in (3, 9, 10, 16)])
    ties = np.array([(x, 19 - x, 10) for x in range(10, 20)] + [(x, 10, 19 - x) for x in range(10, 20)] +  # the mirrored side: within an ulp or two
                    [(x, x, 10) for x in range(10, 20)] + [(x, 10, x) for x in range(10, 20)])            # q_x == q_z, q_y == q_z: exact
    out = [(PERM, 0.0, float(px[15]), 1.0, 1.0, dims, np.concatenate([grid, ties])),                      # q_z == far_z at x = 15
           (PERM, float(px[12]), float(px[17]), 1.0, 1.0, dims, np.concatenate([grid, ties])),            # q_z == near_z at x = 12
           (GENERIC, 0.1, 1.2, 0.83, 0.62, dims, grid),
           (np.where(np.arange(9) == 4, np.nan, PERM), 0.0, 9.0, 1.0, 1.0, dims, grid[:40]),
           (np.where(np.arange(9) == 2, np.inf, PERM), 0.0, 9.0, 1.0, 1.0, dims, grid[:40])]
    return out


def case_text():
    """(input lines, expected output lines)"""
    lines, want = [], []
    rng = np.random.default_rng(0x4d41)
    for L in (1, 63, 64, 65, 66, 128, 130):
        named = sorted({x for x in (0, 63, 64, L - 1) if x < L})
        rows = [[x] for x in named] + [named, list(np.nonzero(rng.random(L) < 0.1)[0]), list(range(L)), []]
        for r in range(4):
            for xs in rows:
                w = words_of([int(x) for x in xs], L)
                lines.append(f"D {L} {r} {len(w)} " + " ".join(f"{v:016x}" for v in w))
                want.append("D " + " ".join(f"{v:016x}" for v in mref.dilate_row_words(w, L, r)))
    f = np.float32
    up = lambda v: np.nextafter(f(v), f(np.inf))                                                  # noqa: E731
    for v, t in [(0.2, 0.2), (up(0.2), 0.2), (np.nextafter(f(0.2), f(-np.inf)), 0.2), (np.nan, 0.2), (0.5, np.nan), (-0.0, 0.0),
                 (0.0, -0.0), (up(0.0), 0.0), (np.inf, 3e38), (-np.inf, -3e38), (1.0, 0.0), (f(np.float16(0.2)), 0.2)]:
        lines.append(f"O {h32(v)} {h32(t)}")
        want.append(f"O {int(mref.occupied(f(v), f(t)))}")
    for rot, near, far, th, tv, dims, cells in frustum_cases():
        p = mref.centres(dims, RES)
        rngs = [f(n // 2) * RES for n in dims]
        for ix, iy, iz in cells:
            lines.append(f"F {h64(rot)} {h64([near, far, th, tv])} {h32([RES, *rngs])} {ix} {iy} {iz}")
            ok = mref.in_view(p[0][ix], p[1][iy], p[2][iz], rot, near, far, th, tv)
            want.append(f"F {int(ok)} {h64([p[0][ix], p[1][iy], p[2][iz]])}")
    for L, W, H in ((100, 100, 100), (66, 66, 20), (130, 6, 8), (300, 300, 300), (1, 1, 1), (4096, 2048, 4), (1024, 1024, 16)):
        for r in range(4):
            for slab in (0, 1, 2, 3, 7, 64, 10 ** 6):
                lines.append(f"Y {L} {W} {H} {r} {slab}")
                got = mref.layout(L, W, H, r, slab)
                want.append("Y " + " ".join(str(v) for v in got) + " carved")
    return lines, want


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "mapaudit_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "mapaudit_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "mapaudit")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "mapaudit_san")
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    return out


@pytest.fixture(scope="module")
def expected():
    return case_text()


def check_all(exe, tmp_path, expected):
    lines, want = expected
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    bad = [(lines[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:3])
    kinds = {k: sum(1 for w in want if w.startswith(k)) for k in ("D", "O 0", "O 1", "F 0", "F 1", "Y")}
    print("lines per kind:", kinds)
    assert all(v > 0 for v in kinds.values()) and kinds["F 1"] > 100


def test_host_bodies_equal_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_bodies_run_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


def test_the_named_cases_are_what_they_are_named_for():
    """the ties are exact ties and are in view; near_z itself is out, far_z itself is in; a NaN or inf rotation sees nothing;
    the layout keeps within the LDS and refuses what cannot fit"""
    cases = frustum_cases()
    rot, near, far, th, tv, dims, cells = cases[0]
    p = mref.centres(dims, RES)
    ties = cells[-20:]
    assert all(abs(p[1][y]) == p[0][x] or abs(p[2][z]) == p[0][x] for x, y, z in ties)
    seen = np.array([mref.in_view(p[0][x], p[1][y], p[2][z], rot, near, far, th, tv) for x, y, z in ties])
    assert seen[[x <= 15 for x, _, _ in ties]].all() and not seen[[x > 15 for x, _, _ in ties]].any()
    assert mref.in_view(p[0][15], p[1][10], p[2][10], rot, near, far, th, tv)                       # q_z == far_z: in
    rot, near, far, th, tv, _, _ = cases[1]
    assert near == p[0][12] and not mref.in_view(p[0][12], p[1][10], p[2][10], rot, near, far, th, tv)   # q_z == near_z: out
    assert mref.in_view(p[0][13], p[1][10], p[2][10], rot, near, far, th, tv)
    for k in (3, 4):
        assert not mref.region((20, 20, 20), RES, None, cases[k][:5]).any()
    assert 0 < mref.region((20, 20, 20), RES, None, cases[2][:5]).sum() < 8000
    for L, W, H in ((100, 100, 100), (300, 300, 300), (1024, 1024, 16)):
        for r in range(4):
            lay = mref.layout(L, W, H, r, 10 ** 6)
            assert lay[6] <= 159 * 1024 and (lay[3] == H or 8 * lay[1] * (lay[3] + 1 + (4 if r else 2) * (lay[3] + 1 + 2 * r)) > 159 * 1024)
    assert mref.layout(4096, 2048, 4, 0, 0)[3] == 0 and mref.layout(100, 100, 100, 1, 0)[3] == 4


# ---- 2. the reading against pairwise distances ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims,density", [((21, 17, 9), 0.02), ((30, 11, 13), 0.2), ((66, 5, 6), 0.5), ((12, 12, 12), 0.0)])
def test_the_reading_against_brute_force_chebyshev(dims, density):
    L, W, H = dims
    rng = np.random.default_rng(L * 1000 + W)
    T = 3
    test = (rng.random((L * W * H, T)) < density).astype(np.float32)
    truth = (rng.random((L * W * H, T)) < density * 0.7).astype(np.float32) * 0.9
    assert (test > 0.5).sum() <= 2000 * T and (truth > 0.5).sum() <= 2000 * T
    box = ((2, 1, 1), (L - 3, W - 1, H - 2))
    fr = (GENERIC, 0.05, 1.6, 0.9, 0.7)
    for r in range(4):
        for b, f in ((None, None), (box, None), (box, fr)):
            rows = mref.audit_agent(test, truth, dims, RES, 0.5, 0.5, r, b, f)
            R = mref.region(dims, RES, b, f)
            vt, vg = mref.volume(test, dims) > 0.5, mref.volume(truth, dims) > 0.5
            for t in range(T):
                want = [R.sum(), (vt[t] & R).sum(), (vg[t] & R).sum(), mref.brute_force_near(vt[t], vg[t], R, 0),
                        mref.brute_force_near(vt[t], vg[t], R, r), mref.brute_force_near(vg[t], vt[t], R, r)]
                assert rows[t, :6].tolist() == [int(v) for v in want], (r, t, rows[t], want)
                assert rows[t, 6] == t and rows[t, 7] == 0
            if r == 0:
                assert (rows[:, 4] == rows[:, 3]).all() and (rows[:, 5] == rows[:, 3]).all()
    if density > 0:
        assert rows[:, 4].sum() > rows[:, 3].sum()                       # r = 3 finds more than r = 0


def test_the_reading_skips_and_refuses_as_the_header_says():
    dims = (6, 5, 4)
    g = np.ones((120, 3), np.float32)
    rows = mref.audit_agent(g, g[:, :2], dims, RES, 0.5, 0.5, 1, slice_map=[1, -1, 0])
    assert rows[:, 6].tolist() == [1, -1, 0] and rows[:, 7].tolist() == [0, mref.SKIPPED, 0] and not rows[1, :6].any()
    assert rows[0, :6].tolist() == [120] * 6
    rows = mref.audit_agent(g, g, dims, RES, 0.5, 0.5, 1, centre_test=[0, 0, 0], centre_truth=[0, -0.0, 0])
    assert (rows[:, 7] == mref.CENTRE).all() and not rows[:, :6].any()
    assert mref.audit_agent(g, g[:, :2], dims, RES, 0.5, 0.5)[:, 6].tolist() == [0, 1, -1]     # the default slice_map


# ---- 3. the entry ------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound(pop):
    txt = open(os.path.join(ROOT, "include", "sogm_abi.h")).read()
    lib = C.CDLL(pop._abi.LIB_PATH)
    for name in ("sogm_map_audit", "sogm_map_audit_default_params"):
        assert f"int {name}(" in txt and hasattr(lib, name) and name in pop._abi.PROTOTYPES
    assert "SOGM_ABI_VERSION 6" in txt and pop.lib().sogm_abi_version() == 6
    assert C.sizeof(pop._abi.SogmMapAuditParams) == 208 and "/* 208 bytes */" in txt
    assert pop._abi.SogmMapAuditParams.slice_map.offset == 80 and pop._abi.SogmMapAuditParams.near_z.offset == 48


def test_default_params(pop):
    lib, bad = pop.lib(), pop._abi.SOGM_ERR_INVALID_ARG
    prm = pop._abi.SogmMapAuditParams()
    C.memset(C.byref(prm), 0xA5, C.sizeof(prm))
    assert lib.sogm_map_audit_default_params(6, 4, C.byref(prm)) == 0
    assert list(prm.slice_map) == [0, 1, 2, 3] + [-1] * 28
    assert bytes(prm)[:80] == bytes(80)
    assert lib.sogm_map_audit_default_params(3, 15, C.byref(prm)) == 0 and list(prm.slice_map)[:4] == [0, 1, 2, -1]
    for args in ((0, 4), (4, 0), (33, 4), (4, 33)):
        assert lib.sogm_map_audit_default_params(*args, C.byref(prm)) == bad
    assert lib.sogm_map_audit_default_params(6, 6, None) == bad and b"default_params" in lib.sogm_last_error()


def test_null_pointers_and_own_fields_are_refused_before_anything_else(pop):
    """with pointers that are never dereferenced: the refusals that need no context come first"""
    lib, bad = pop.lib(), pop._abi.SOGM_ERR_INVALID_ARG
    prm = pop._abi.SogmMapAuditParams()
    assert lib.sogm_map_audit_default_params(6, 6, C.byref(prm)) == 0
    fake = C.create_string_buffer(64)
    ctx, out = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    assert lib.sogm_map_audit(None, ctx, C.byref(prm), None, out, None, None) == bad
    assert b"sogm_map_audit: null pointer" in lib.sogm_last_error()
    assert lib.sogm_map_audit(ctx, None, C.byref(prm), None, out, None, None) == bad
    assert lib.sogm_map_audit(ctx, ctx, None, None, out, None, None) == bad
    assert lib.sogm_map_audit(ctx, ctx, C.byref(prm), None, None, None, None) == bad
    for tol in (-1, 4):
        prm.tolerance = tol
        assert lib.sogm_map_audit(ctx, ctx, C.byref(prm), None, out, None, None) == bad and b"tolerance" in lib.sogm_last_error()
    prm.tolerance = 0
    prm.flags = pop._abi.SOGM_MAPAUDIT_FRUSTUM
    prm.near_z, prm.far_z, prm.tan_h, prm.tan_v = 0.0, 5.0, 1.0, 1.0
    assert lib.sogm_map_audit(ctx, ctx, C.byref(prm), None, out, None, None) == bad and b"cam_rot" in lib.sogm_last_error()
    for field, v in (("near_z", np.nan), ("far_z", np.inf), ("tan_h", np.nan), ("tan_v", -np.inf), ("near_z", -0.1), ("far_z", 0.0),
                     ("tan_h", 0.0), ("tan_v", -1.0)):
        keep = getattr(prm, field)
        setattr(prm, field, v)
        assert lib.sogm_map_audit(ctx, ctx, C.byref(prm), out, out, None, None) == bad, (field, v)
        setattr(prm, field, keep)


def test_without_a_gpu_the_entry_fails_loudly(pop):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = pop.lib()
    prm = pop._abi.SogmMapAuditParams()
    assert lib.sogm_map_audit_default_params(6, 6, C.byref(prm)) == 0
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    assert lib.sogm_map_audit(p, p, C.byref(prm), None, p, None, None) == pop._abi.SOGM_ERR_NO_DEVICE
    assert b"no HIP device" in lib.sogm_last_error()


def test_facade_audit_against_compiles_and_refuses(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "mapaudit_facade_host_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "mapaudit_facade_host_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "map audit facade host ok" in out.stdout
