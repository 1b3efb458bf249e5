"""CPU: the view mask (include/sogm_abi.h "view mask") without a GPU.
  1. the body of csrc/sogm_viewmask.hpp, compiled with the host compiler (tests/view_rules_host_test.cpp), against the numpy
     reading of the header (tests/view_mask_reference.py), class for class and word for word: the three cyclic axis
     permutations (every value exact), a generic yaw plus pitch, a NaN rotation, exact ties on every comparison, uf + 0.5 and
     vf + 0.5 exactly an integer at both image edges, d16 in {0, 1, 65535}, cam_offset NULL, zero and non-zero, L = 70 (six
     live bits in a row's last word).  The same program under -fsanitize=address,undefined runs them clean;
  2. the hand-built inputs are what they are named for, and every batch makes every class non-empty (the GPU test
     tests/test_view_mask_gpu.py runs the same batches: it cannot pass on an all-OUTSIDE volume);
  3. the entries: declared, exported, bound; null pointers and prm's own fields refused; no device, said loudly."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import view_mask_reference as vref  # noqa: E402
from test_map_audit_host import GENERIC, PERM, h32, h64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 24, 32
P1 = PERM.reshape(3, 3)
PERMS = [PERM, (P1 @ P1).reshape(9), (P1 @ P1 @ P1).reshape(9)]          # q_z = p_0;  q_z = p_1;  the identity: q_z = p_2
NAN_ROT = np.where(np.arange(9) == 4, np.nan, PERM)


def image(wall, step, one=None, big=None, flip=False):
    """24 x 32: a far wall everywhere, a nearer step over the left half (the edge runs between columns 15 and 16), a block of
    zeros (no return) at rows 8 .. 15, columns 20 .. 27, and optionally single pixels of 1 and 65535"""
    d = np.full((ROWS, COLS), wall, np.uint16)
    d[:, :16] = step
    d[8:16, 20:28] = 0
    if one is not None:
        d[one] = 1
    if big is not None:
        d[big] = 65535
    return np.ascontiguousarray(d[::-1, ::-1]) if flip else d


def params(band, near=0.0, far=8.25, tan_h=1.0, tan_v=1.0, fx=16.0, fy=16.0, cx=15.5, cy=11.5, scale=1000.0, max_depth=20.0):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, depth_scale=scale, max_depth=max_depth, near_z=near, far_z=far, tan_h=tan_h,
                tan_v=tan_v, band=band, rows=ROWS, cols=COLS)


def batches():
    """name -> (dims, res, prm, depths [n, 24, 32], rots [n, 9], offsets [n, 3] or None).  The long grid has res = 0.5: every
    centre is an odd multiple of 0.25; with depth_scale 1000 and d16 in multiples of 250, z_hit and z_hit +- band are exact."""
    long_, cube = (70, 5, 6), (16, 16, 16)
    img = image(4250, 2000, one=(13, 17), big=(12, 15))
    out = {}
    for band in (0.0, 0.25):
        out[f"perms band {band}"] = (long_, 0.5, params(band), np.stack([img, image(4250, 2000, flip=True), image(250, 0)]),
                                     np.stack(PERMS), None)
    out["offset zero"] = (long_, 0.5, params(0.25), np.stack([img, img]), np.stack([PERM, PERM]), np.zeros((2, 3)))
    # q_z = 0.5 i - 17.5 (whole and half metres): q_z = 1 with q_y = +-0.75 puts vf + 0.5 on an integer at both image edges
    out["offset"] = (long_, 0.5, params(0.0, tan_v=0.75), np.stack([image(4000, 2000), img]), np.stack([PERM, PERM]),
                     np.array([[0.25, 0.0, 0.0], [-0.5, 0.25, 0.0]]))
    small = params(0.15, far=1.1, tan_h=1.3, tan_v=0.95)                   # wider than the image (1.0, 0.75): OFFIMAGE cells
    out["cube"] = (cube, 0.15, small, np.stack([image(800, 450), image(700, 300, flip=True), image(800, 450)]),
                   np.stack([GENERIC, PERM, NAN_ROT]), np.array([[0.013, -0.027, 0.031], [-0.2, 0.05, 0.0], [0.0, 0.0, 0.0]]))
    out["cube no offset"] = (cube, 0.15, dict(small, band=0.075), np.stack([image(800, 450), image(700, 300, one=(12, 18))]),
                             np.stack([PERM, GENERIC]), None)
    return out


def reading(batch, classes):
    dims, res, prm, depths, rots, offs = batch
    return vref.view_mask(dims, np.float32(res), depths, rots, prm, classes, offs)


def case_text():
    """(input lines, expected output lines): every agent of every batch, classes = all and FREE | SURFACE"""
    lines, want = [], []
    for name, batch in batches().items():
        dims, res, prm, depths, rots, offs = batch
        rngs = [np.float32(n // 2) * np.float32(res) for n in dims]
        for classes in (vref.ALL, vref.BIT[vref.FREE] | vref.BIT[vref.SURFACE]):
            cls, words, counts = reading(batch, classes)
            for a in range(len(depths)):
                off = np.zeros(3) if offs is None else offs[a]
                nums = [prm[k] for k in ("fx", "fy", "cx", "cy", "depth_scale", "near_z", "far_z", "tan_h", "tan_v", "band")]
                lines.append(f"V {dims[0]} {dims[1]} {dims[2]} {h32([np.float32(res), *rngs])} {h64(rots[a])} "
                             f"{0 if offs is None else 1} {h64(off)} {h64(nums)} {ROWS} {COLS} {classes} " +
                             " ".join(f"{int(v):x}" for v in depths[a].reshape(-1)))
                want.append("C " + "".join(str(int(c)) for c in cls[a].reshape(-1)))
                want.append("W " + " ".join(f"{int(w):016x}" for w in words[a].reshape(-1)) + " N " +
                            " ".join(str(int(v)) for v in counts[a, :6]))
    return lines, want


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "view_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "view_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "viewmask")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "viewmask_san")
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
    assert len(got) == len(want) == 2 * len(lines)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = next(j for j in range(min(len(g), len(w))) if g[j] != w[j]) if len(g) == len(w) else -1
            raise AssertionError((lines[i // 2][:60], "line", i, "first difference at", k, g[max(k - 8, 0):k + 8], w[max(k - 8, 0):k + 8]))


def test_host_body_equals_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_body_runs_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


def test_host_program_reads_stdin_too(exe, expected):
    lines, want = expected
    run = subprocess.run([exe], input=lines[0] + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.splitlines() == want[:2]


# ---- 2. the inputs are what they are named for -------------------------------------------------------------------------------
def test_every_batch_makes_every_class_non_empty():
    for name, batch in batches().items():
        cls, words, counts = reading(batch, vref.ALL)
        dims = batch[0]
        print(name, counts[:, :6].tolist())
        assert (counts[:, :5].sum(axis=0) > 0).all(), (name, counts[:, :5].sum(axis=0))
        assert (counts[:, :5].sum(axis=1) == dims[0] * dims[1] * dims[2]).all() and (counts[:, 5] == counts[:, :5].sum(axis=1)).all()
        assert not counts[:, 6:].any()
    cls = reading(batches()["cube"], vref.ALL)[0]
    assert (cls[2] == vref.OUTSIDE).all()                                 # the NaN rotation sees nothing
    assert all(len(np.unique(cls[a])) == 5 for a in (0, 1))               # and each other agent alone has all five


def test_spare_bits_and_layout():
    """L = 70: the second word of a row has six live bits; with every class selected exactly those are set"""
    _, words, counts = reading(batches()["perms band 0.0"], vref.ALL)
    assert words.shape == (3, 6, 5, 2) and (words[..., 0] == np.uint64(2 ** 64 - 1)).all() and (words[..., 1] == np.uint64(63)).all()
    bits = np.zeros((2, 3, 70), bool)
    bits[1, 2, [0, 63, 64, 69]] = True
    w = vref.pack(bits)
    assert w[1, 2].tolist() == [1 | 1 << 63, 1 | 1 << 5] and not w[0].any() and np.array_equal(vref.unpack(w, 70), bits)


def test_the_ties_are_ties_and_fall_as_the_header_says():
    """PERM on the long grid: q_z = p_0 = 0.5 ix - 17.25, q_x = p_1 = 0.5 iy - 0.75, q_y = p_2 = 0.5 iz - 1.25"""
    b = batches()
    dims, res, prm, depths, rots, _ = b["perms band 0.25"]
    px, py, pz = vref.cell_centres(dims, np.float32(res))
    assert px[35] == 0.25 and py[1] == -0.25 and pz[3] == 0.25 and px[51] == prm["far_z"]
    cls = reading(b["perms band 0.25"], vref.ALL)[0][0]                    # agent 0, [z, y, x]
    # the step (z_hit = 2.0) is seen by the cells left of the axis (iy = 0, 1): 1.75 == z_hit - band and 2.25 == z_hit + band
    assert depths[0][13, 14] == 2000 and px[38] == 1.75 and px[39] == 2.25
    assert cls[3, 1, 37:41].tolist() == [vref.FREE, vref.SURFACE, vref.SURFACE, vref.HIDDEN]
    # the wall (4.25) right of the axis: one SURFACE cell strictly inside the band, the cells beyond it HIDDEN up to far_z
    assert cls[2, 2, 42:45].tolist() == [vref.FREE, vref.SURFACE, vref.HIDDEN] and cls[2, 2, 51] == vref.HIDDEN
    assert cls[2, 2, 52] == vref.OUTSIDE                                   # q_z == far_z is in, the next cell is out
    cls0 = reading(b["perms band 0.0"], vref.ALL)[0][0]
    assert px[43] == 4.25 and cls0[2, 2, 42:45].tolist() == [vref.FREE, vref.SURFACE, vref.HIDDEN]   # q_z == z_hit, band 0
    # the frustum's own edge |q_x| == q_z tan_h is in view; there uf + 0.5 is exactly 0 on the left (u = 0: on the image)
    # and exactly cols on the right (off it)
    assert px[36] == 0.75 and py[0] == -0.75 and py[3] == 0.75
    assert cls[2, 0, 36] in (vref.FREE, vref.SURFACE, vref.HIDDEN) and cls[2, 3, 36] == vref.OFFIMAGE
    assert (-0.75 / 0.75) * prm["fx"] + prm["cx"] + 0.5 == 0.0 and (0.75 / 0.75) * prm["fx"] + prm["cx"] + 0.5 == COLS
    # d16 = 1 hides everything behind one pixel, 65535 frees everything in front of another, a zero frees as well
    assert depths[0][13, 17] == 1 and depths[0][12, 15] == 65535
    assert (cls[3, 2, 39:43] == vref.HIDDEN).all() and (cls[3, 1, 43:52] == vref.FREE).all()
    assert cls[2, 4, 44] == vref.FREE and cls[2, 4, 45] == vref.HIDDEN and depths[0][11, 20] == 0           # behind the wall's depth, but through the zero block
    # the vertical edges, with the offset batch: q_z = 1.0 at ix = 37, q_y = -+0.75 at iz = 1, 4
    dims, res, prm, depths, rots, offs = b["offset"]
    cls = reading(b["offset"], vref.ALL)[0][0]
    p = vref.cell_centres(dims, np.float32(res), offs[0])
    assert p[0][37] == 1.0 and p[2][1] == -0.75 and p[2][4] == 0.75
    assert (-0.75 / 1.0) * prm["fy"] + prm["cy"] + 0.5 == 0.0 and (0.75 / 1.0) * prm["fy"] + prm["cy"] + 0.5 == ROWS
    assert cls[1, 1, 37] >= vref.FREE and cls[4, 1, 37] == vref.OFFIMAGE
    # a zero offset is not a missing offset in the rule, but gives the same classes here (no centre of this grid is -0.0)
    z, n = reading(b["offset zero"], vref.ALL), reading(b["perms band 0.25"], vref.ALL)
    assert np.array_equal(z[0][0], n[0][0])


# ---- 3. the entries ----------------------------------------------------------------------------------------------------------
def good_prm(pop, **kw):
    p = pop._abi.SogmViewParams()
    for k, v in params(0.0).items():
        setattr(p, k, v)
    p.classes = pop._abi.SOGM_VIEWBIT_FREE | pop._abi.SOGM_VIEWBIT_SURFACE
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# every refusal of sogm_view_mask that prm alone can cause
BAD_PRM = [("rows", 0), ("cols", 0), ("cols", -3), ("fx", np.nan), ("fy", np.inf), ("cx", np.nan), ("cy", -np.inf),
           ("depth_scale", np.nan), ("max_depth", np.inf), ("band", np.nan), ("near_z", np.nan), ("far_z", np.inf), ("tan_h", np.nan),
           ("tan_v", np.inf), ("fx", 0.0), ("fy", -1.0), ("depth_scale", 0.0), ("max_depth", 0.0), ("tan_h", 0.0), ("tan_v", -0.5),
           ("near_z", -0.1), ("far_z", 0.0), ("far_z", 20.5), ("band", -0.01), ("classes", 0), ("classes", 32), ("classes", -1)]


def test_the_entries_are_declared_exported_and_bound(pop):
    txt = open(os.path.join(ROOT, "include", "sogm_abi.h")).read()
    lib = C.CDLL(pop._abi.LIB_PATH)
    for name in ("sogm_view_mask", "sogm_view_default_params", "sogm_map_audit_masked"):
        assert f"int {name}(" in txt and hasattr(lib, name) and name in pop._abi.PROTOTYPES
    assert "SOGM_ABI_VERSION 6" in txt and pop.lib().sogm_abi_version() == 6
    assert C.sizeof(pop._abi.SogmViewParams) == 104 and "/* 104 bytes */" in txt
    assert pop._abi.SogmViewParams.band.offset == 80 and pop._abi.SogmViewParams.classes.offset == 96
    a = pop._abi
    assert [a.SOGM_VIEW_OUTSIDE, a.SOGM_VIEW_OFFIMAGE, a.SOGM_VIEW_FREE, a.SOGM_VIEW_SURFACE, a.SOGM_VIEW_HIDDEN] == list(range(5))
    assert [a.SOGM_VIEWBIT_OUTSIDE, a.SOGM_VIEWBIT_OFFIMAGE, a.SOGM_VIEWBIT_FREE, a.SOGM_VIEWBIT_SURFACE,
            a.SOGM_VIEWBIT_HIDDEN] == [1 << c for c in range(5)] and a.SOGM_VIEWBIT_ALL == 31


def test_default_params(pop):
    lib, bad = pop.lib(), pop._abi.SOGM_ERR_INVALID_ARG
    depth = __import__("importlib").import_module("pred-occ-planner_amd.depth")
    cam = depth.make_depth_camera(60, 80, 4.0, 1000.0, fx=48.375, fy=40.0, cx=39.5, cy=29.5)
    prm = pop._abi.SogmViewParams()
    C.memset(C.byref(prm), 0xA5, C.sizeof(prm))
    assert lib.sogm_view_default_params(C.byref(cam), C.byref(prm)) == 0
    assert [prm.fx, prm.fy, prm.cx, prm.cy, prm.depth_scale, prm.max_depth] == [48.375, 40.0, 39.5, 29.5, 1000.0, 4.0]
    assert [prm.near_z, prm.far_z, prm.tan_h, prm.tan_v, prm.band] == [0.0, 4.0, 0.5 * 80 / 48.375, 0.5 * 60 / 40.0, 0.0]
    assert [prm.rows, prm.cols, prm.classes, prm.reserved_] == [60, 80, 4 | 8, 0]
    assert lib.sogm_view_default_params(None, C.byref(prm)) == bad and b"sogm_view_default_params" in lib.sogm_last_error()
    assert lib.sogm_view_default_params(C.byref(cam), None) == bad


def test_null_pointers_and_own_fields_are_refused_before_anything_else(pop):
    """with pointers that are never dereferenced: the refusals that need no context come first"""
    lib, bad = pop.lib(), pop._abi.SOGM_ERR_INVALID_ARG
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    prm = good_prm(pop)
    for k in range(5):
        args = [p, C.byref(prm), p, p, None, p, None, None]
        args[(0, 1, 2, 3, 5)[k]] = None
        assert lib.sogm_view_mask(*args) == bad and b"sogm_view_mask: null pointer" in lib.sogm_last_error(), k
    for field, v in BAD_PRM:
        assert lib.sogm_view_mask(p, C.byref(good_prm(pop, **{field: v})), p, p, p, p, p, None) == bad, (field, v)
        assert lib.sogm_last_error().startswith(b"sogm_view_mask: "), (field, v)
    assert lib.sogm_view_mask(p, C.byref(good_prm(pop, rows=65536, cols=65536)), p, p, p, p, p, None) == bad   # 2^32 pixels
    # the masked audit: a null mask, a set frustum flag, the audit's own tolerance
    ap = pop._abi.SogmMapAuditParams()
    assert lib.sogm_map_audit_default_params(3, 3, C.byref(ap)) == 0
    assert lib.sogm_map_audit_masked(p, p, C.byref(ap), None, p, None, None) == bad
    assert b"sogm_map_audit_masked: null pointer" in lib.sogm_last_error()
    for k in (0, 1, 2, 4):
        args = [p, p, C.byref(ap), p, p, None, None]
        args[k] = None
        assert lib.sogm_map_audit_masked(*args) == bad, k
    ap.flags = pop._abi.SOGM_MAPAUDIT_FRUSTUM
    ap.near_z, ap.far_z, ap.tan_h, ap.tan_v = 0.0, 5.0, 1.0, 1.0
    assert lib.sogm_map_audit_masked(p, p, C.byref(ap), p, p, None, None) == bad and b"FRUSTUM" in lib.sogm_last_error()
    ap.flags = 0
    ap.near_z = np.nan                                      # not read without the flag
    ap.tolerance = 4
    assert lib.sogm_map_audit_masked(p, p, C.byref(ap), p, p, None, None) == bad and b"tolerance" in lib.sogm_last_error()


def test_without_a_gpu_the_entries_fail_loudly(pop):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = pop.lib()
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    assert lib.sogm_view_mask(p, C.byref(good_prm(pop)), p, p, None, p, None, None) == pop._abi.SOGM_ERR_NO_DEVICE
    assert b"sogm_view_mask: no HIP device" in lib.sogm_last_error()
    ap = pop._abi.SogmMapAuditParams()
    assert lib.sogm_map_audit_default_params(3, 3, C.byref(ap)) == 0
    ap.near_z = np.nan
    assert lib.sogm_map_audit_masked(p, p, C.byref(ap), p, p, None, None) == pop._abi.SOGM_ERR_NO_DEVICE
    assert b"sogm_map_audit_masked: no HIP device" in lib.sogm_last_error()


def build_facade_program(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "viewmask_facade_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "viewmask_facade_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    return exe


def test_facade_view_mask_compiles_and_refuses(tmp_path):
    out = subprocess.run([build_facade_program(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "view mask facade ok" in out.stdout
