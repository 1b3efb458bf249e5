"""CPU: ring obstacles (include/sogm_abi.h "ring obstacles") without a GPU.
  1. the bodies of csrc/sogm_ring.hpp, compiled with the host compiler (tests/ring_rules_host_test.cpp), against the two
     numpy readings of the header (tests/depth_ring_reference.py, tests/audit_ring_reference.py), bit for bit, on the
     fixture rays and poses; the same program under -fsanitize=address,undefined runs them clean;
  2. the ray rule against exact quartic roots, the box rule against 65 536 sampled circle points;
  3. what the fixtures are named for, and the flag-clear reading."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_ring_reference as ringaudit  # noqa: E402
import depth_render_reference as cylref  # noqa: E402
import depth_ring_reference as ringref  # noqa: E402
import ring_fixtures as fx  # noqa: E402
import swarm_audit_reference as aref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = (0.4, 0.4, 0.45)


def hexes(v):
    return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(v, np.float64).reshape(-1).view(np.uint64))


def rec_text(row):
    return f"{int(row[0])} " + hexes(row[1:])


def ray_cases():
    """(record row, p [3], d [n, 3]) per (camera, valid ring) of the branch scene at 37 x 53: every 5th pixel, and the whole
    row with yc == 0"""
    rec, cam, pos, rot = fx.branch_scene(37, 53)
    out = []
    for a in range(len(pos)):
        d, _, _ = ringref.rays(cam, rot[a])
        d = np.stack([x.reshape(-1) for x in d], axis=1)
        pick = np.zeros(cam.rows * cam.cols, bool)
        pick[::5] = True
        pick[(cam.rows // 2) * cam.cols:(cam.rows // 2 + 1) * cam.cols] = True
        for row in rec:
            if row[0] == 2 and ringref.frame(row) is not None:
                out.append((row, pos[a], d[pick]))
    return out


def case_text():
    rec, _, _, _ = fx.branch_scene()
    lines = ["T"]
    lines += ["F " + rec_text(r) for r in rec]
    bad = np.array(fx.ring(1.0, 2.0, 3.0, 1.0))
    for k, v in ((1, np.nan), (4, np.inf), (6, -np.inf), (4, 0.0), (5, 0.0), (4, -1.0), (8, 1e200)):
        r = bad.copy()
        r[k] = v
        if k == 8:
            r[9] = 1e200                                  # |q| overflows
        lines.append("F " + rec_text(r))
    for row, p, d in ray_cases():
        head = "R " + rec_text(row) + " " + hexes(p) + " "
        lines += [head + hexes(x) for x in d]
    for row, a in fx.audit_poses():
        head = "G " + rec_text(row) + " "
        lines += [head + hexes(x) + " " + hexes(BODY) for x in a]
    return "\n".join(lines) + "\n", lines


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "ring_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "ring_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "ring")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ring_san")
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    return out


@pytest.fixture(scope="module")
def expected():
    """the readings' answers to case_text(), line by line"""
    text, lines = case_text()
    want = []
    rays = iter(ray_cases())
    poses = iter(fx.audit_poses())
    i = 0
    while i < len(lines):
        tag = lines[i][0]
        if tag == "T":
            want.append("T " + hexes(ringaudit.TABLE))
            i += 1
        elif tag == "F":
            f = lines[i].split()
            row = np.concatenate([[float(f[1])], np.array([int(v, 16) for v in f[2:]], np.uint64).view(np.float64)])
            fr = ringref.frame(row)
            want.append("F 0" if fr is None else "F 1 " + hexes([fr[1], fr[2], *fr[3], *fr[4], *fr[5]]))
            i += 1
        elif tag == "R":
            row, p, d = next(rays)
            c, R, rho, _, _, n = ringref.frame(row)
            t, _ = ringref.ray_hit(p, [d[:, 0], d[:, 1], d[:, 2]], c, R, rho, n)
            want += [f"R {int(np.isfinite(x))} " + hexes(x if np.isfinite(x) else 0.0) for x in t]
            i += len(d)
        else:
            row, a = next(poses)
            c, R, rho, e1, e2, _ = ringref.frame(row)
            gap = ringaudit.box_gap(np.tile(c, (len(a), 1)), R, rho, e1, e2, a, BODY)
            want += ["G " + hexes(g) for g in gap]
            i += len(a)
    return text, want


def check_all(exe, tmp_path, expected):
    text, want = expected
    path = tmp_path / "cases.txt"
    path.write_text(text)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:3])
    kinds = {k: sum(1 for w in want if w.startswith(k)) for k in ("F 0", "F 1", "R 0", "R 1", "G")}
    print("lines per kind:", kinds)
    assert all(v > 0 for v in kinds.values()) and kinds["R 1"] > 300


def test_host_bodies_equal_the_two_readings(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_bodies_run_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


def test_the_table_is_the_unit_circle_in_angular_order():
    t = ringaudit.TABLE
    assert np.allclose(np.hypot(t[:, 0], t[:, 1]), 1.0, atol=1e-15)
    ang = np.unwrap(np.arctan2(t[:, 1], t[:, 0]))
    assert np.allclose(np.diff(ang), 2 * np.pi / 64, atol=1e-14)


# ---- 2. accuracy ---------------------------------------------------------------------------------------------------------
def test_the_ray_rule_against_exact_quartic_roots():
    """At most 0.5 % of the pixels the exact roots hit may differ in uint16, and each of those is a miss or a far-side return
    of the same ring whose exact near root lies in a sub-interval with both ends outside.  Observed on these six views:
    see the printed share (DESIGN section 3.3 records it)."""
    n_exact = n_diff = n_extra = 0
    for rec, cam, p, rot in fx.accuracy_views():
        c, R, rho, _, _, n = ringref.frame(rec[0])
        d, _, _ = ringref.rays(cam, rot)
        t, (t0, t1, live) = ringref.ray_hit(p, d, c, R, rho, n)
        co = ringref.coefficients(p, d, c, R, rho, n)[5]
        f = lambda x, v, u: (((co[0][v, u] * x + co[1][v, u]) * x + co[2][v, u]) * x + co[3][v, u]) * x + co[4][v, u]  # noqa: E731
        quant = lambda x: int(np.floor(x * cam.depth_scale + 0.5)) if np.isfinite(x) and x <= cam.max_depth else 0  # noqa: E731
        for v, u in zip(*np.nonzero(live)):
            te = ringref.exact_hit(p, [d[0][v, u], d[1][v, u], d[2][v, u]], c, R, rho, n)
            if not np.isfinite(te):
                n_extra += int(np.isfinite(t[v, u]))
                continue
            n_exact += 1
            if quant(te) == quant(t[v, u]):
                continue
            n_diff += 1
            if not np.isfinite(t[v, u]):
                continue                                   # a miss
            assert t[v, u] > te, "the rule returned a point in front of the exact entry"
            hs = (t1[v, u] - t0[v, u]) / 32.0
            nodes = np.array([t0[v, u]] + [t0[v, u] + i * hs for i in range(1, 32)] + [t1[v, u]])
            i = int(np.searchsorted(nodes, te)) - 1
            assert 0 <= i < 32 and f(nodes[i], v, u) > 0 and f(nodes[i + 1], v, u) > 0, "not a grazing crossing between two nodes"
    share = n_diff / n_exact
    print(f"exact hits {n_exact}, differing {n_diff} ({100 * share:.3f} %), hits where the exact roots see none {n_extra}")
    assert n_exact > 1500
    assert share <= 0.005


def test_the_box_rule_against_65536_circle_points():
    """never below the dense value by more than pi R / 65 536 + 1e-9, never above it by more than 2.5 mm; no collision
    decision within 1e-9 of its threshold, none flipped"""
    worst_above = worst_below = 0.0
    margins = []
    for row, a in fx.audit_poses():
        c, R, rho, e1, e2, _ = ringref.frame(row)
        gap = ringaudit.box_gap(np.tile(c, (len(a), 1)), R, rho, e1, e2, a, BODY)
        margins.append(np.abs(gap))
        for i in range(len(a)):
            dense = ringaudit.dense_gap(c, R, rho, e1, e2, a[i], BODY)
            worst_above, worst_below = max(worst_above, gap[i] - dense), max(worst_below, dense - gap[i])
            assert dense - gap[i] <= np.pi * R / 65536 + 1e-9, (i, gap[i], dense)
            assert gap[i] - dense <= 2.5e-3, (i, gap[i], dense)
            assert (gap[i] < 0) == (dense < 0) or abs(dense) <= np.pi * R / 65536
    print(f"rule above dense by at most {worst_above:.3e} m, below by at most {worst_below:.3e} m")
    assert aref.near_threshold(margins) == 0
    assert sum(int((m < 0.1).sum()) for m in margins) > 30     # poses near the threshold exist


# ---- 3. the fixtures and the flag ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def branch():
    rec, cam, pos, rot = fx.branch_scene()
    return rec, cam, pos, rot, ringref.render_agents(rec, cam, pos, rot, rings=True)


def test_flag_clear_is_the_existing_reading(branch):
    rec, cam, pos, rot, _ = branch
    got = ringref.render_agents(rec, cam, pos, rot, rings=False)
    want = cylref.render_agents(rec[:, :6], cam, pos, rot)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and (got[2] == 12).all()


def test_the_branch_scene_shows_what_its_records_are_named_for(branch):
    rec, cam, pos, rot, (depth, _, unsupported) = branch
    assert (unsupported == 3).all()                        # records 10, 11 (not rings) and 12 (another type)

    def alone(i, a):
        """ring i alone from camera a: t per pixel and the interval"""
        c, R, rho, _, _, n = ringref.frame(rec[i])
        d, _, _ = ringref.rays(cam, rot[a])
        return ringref.ray_hit(pos[a], d, c, R, rho, n), ringref.coefficients(pos[a], d, c, R, rho, n)

    mid = cam.rows // 2
    (t2, (_, _, live2)), co2 = alone(2, 0)
    assert (co2[4][mid] == 0).all() and np.isfinite(t2[mid]).any()           # nd == 0, inside the slab: hits
    (t3, (_, _, live3)), co3 = alone(3, 0)
    assert (co3[4][mid] == 0).all() and not live3[mid].any() and np.isfinite(t3).any()   # nd == 0 outside: that row sees nothing
    (t1, _), co1 = alone(1, 0)
    assert np.isfinite(t1).sum() > 20 and np.abs(co1[4][np.isfinite(t1)]).max() < 0.1   # the optical axis in the ring's plane
    (t4, _), co4 = alone(4, 1)
    assert np.isfinite(t4).sum() > 20                                         # seen from above
    (t0, (s0, _, l0)), _ = alone(0, 2)
    assert (s0[l0] == 0).all() and np.isfinite(t0).sum() > 50                 # inside the sphere: every interval starts at 0
    (t13, _), _ = alone(1, 3)
    assert not np.isfinite(t13).any()                                         # inside the tube: no return from that ring
    assert not np.isfinite(alone(5, 0)[0][0]).any()                           # behind
    t6 = alone(6, 0)[0][0]
    assert np.isfinite(t6).any() and (t6[np.isfinite(t6)] > cam.max_depth).all()   # beyond max_depth
    only_cyl = cylref.render(rec[:, :6], cam, pos[0], rot[0])[0]
    t_r0, t_r8 = alone(0, 0)[0][0], alone(8, 0)[0][0]
    q0 = np.where(np.isfinite(t_r0), np.floor(t_r0 * 1000 + 0.5), 0)
    q8 = np.where(np.isfinite(t_r8) & (t_r8 <= cam.max_depth), np.floor(t_r8 * 1000 + 0.5), 0)
    assert ((q0 > 0) & (only_cyl > q0) & (depth[0] == q0)).sum() > 5           # a ring in front of the cylinder
    assert ((q8 > 0) & (only_cyl > 0) & (only_cyl < q8) & (depth[0] == only_cyl)).sum() > 5   # and one behind it
    t9 = alone(9, 0)[0][0]
    q9 = np.where(np.isfinite(t9), np.floor(t9 * 1000 + 0.5), 0)
    assert ((q9 > 0) & (depth[0] == q9)).sum() > 5 and ((q9 > 0) & (depth[0] < q9) & (depth[0] == only_cyl)).sum() > 0  # cut by the ground
    assert (depth != cylref.render_agents(rec[:, :6], cam, pos, rot)[0]).sum() > 500
