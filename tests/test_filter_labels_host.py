"""CPU: ground-truth labels through the voxel filter (include/sogm_abi.h "ground-truth labels") without a GPU.
  1. the rules of csrc/sogm_labels.hpp, compiled with the host compiler (tests/label_rules_host_test.cpp), against the numpy
     reading of the header (tests/filter_labels_reference.py), bit for bit, on cases named for what they hold; the same program
     under -fsanitize=address,undefined runs them clean;
  2. the named cases do what they are named for, on the reading;
  3. the reading against a different algorithm: a plain loop over a dict of leaves against the vectorised reading;
  4. the hand-built clouds of the GPU test: every named leaf is won by the code it is named for."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_labels_fixtures as lf  # noqa: E402
import filter_labels_reference as lref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def zbits(z):
    return f"{int(np.array([z], f32).view(np.uint32)[0]):08x}"


def hex64(v):
    return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(v, np.float64).reshape(-1).view(np.uint64))


# ---- the named cases ------------------------------------------------------------------------------------------------------
# z from the most negative to the most positive finite fp32: the keys must rise strictly along this list
Z_ORDER = [-3.4e38, -3.5, np.nextafter(f32(-3.5), f32(0)), -1.0, -1e-38, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 0.9999999, 1.0, 3.5, 3.4e38]
ROUND_TRIP_CODES = [-2, -1, 0, 1, 7, INT_MAX, INT_MIN]
WINNERS = [
    ("equal z with two codes: the larger", [(1.5, 3), (1.5, 7)], 7),
    ("equal z with two codes, the other order", [(1.5, 7), (1.5, 3)], 7),
    ("z decides against the larger code", [(1.5, 9), (1.25, 0)], 0),
    ("a body over a record over the ground over none", [(2.0, 1), (2.0, lf.HIT_NONE), (2.0, 4), (2.0, lf.HIT_GROUND)], 4),
    ("a record over the ground", [(2.0, lf.HIT_GROUND), (2.0, 0)], 0),
    ("-0 before +0", [(0.0, 100), (-0.0, lf.HIT_GROUND)], lf.HIT_GROUND),
    ("negative z before -0", [(-0.0, 5), (-1e-45, 2)], 2),
    ("one ulp of z decides", [(float(np.nextafter(f32(2.0), f32(3))), 9), (2.0, 0)], 0),
    ("INT_MAX over everything at equal z", [(1.0, 5), (1.0, INT_MAX), (1.0, INT_MIN)], INT_MAX),
]


def _ulp_above_case():
    """a body velocity whose s2 is min_speed^2 = 0.25 and one whose s2 is the next fp32 above it"""
    vy = f32(1.5 * 2.0 ** -13)
    s2 = f32(0.5) * f32(0.5) + vy * vy
    assert s2 == np.nextafter(f32(0.25), f32(1)) and f32(0.5) * f32(0.5) == f32(0.25)
    return [[0.5, 0.0, 0.0], [0.5, float(vy), 0.0], [0.0, 0.0, 0.5], [0.0, float(vy), 0.5]]


# (name, min_speed, records' (vx, vy), bodies' velocities, [(what, code, is a label expected)])
SOURCES = [
    ("the GPU test's sources", lf.MIN_SPEED, lf.REC[:, 6:8], lf.BODY_VEL,
     [("record", 0, True), ("record at rest", 1, False), ("type-2 record", 2, True), ("body", 3, True), ("body at rest", 4, False),
      ("body below min_speed", 5, False), ("ground", lf.HIT_GROUND, False), ("none", lf.HIT_NONE, False),
      ("at n_cyl + n_bodies", 6, False), ("beyond", 11, False), ("INT_MAX", INT_MAX, False), ("INT_MIN", INT_MIN, False), ("-3", -3, False)]),
    ("s2 against min_speed^2", 0.5, [[0.5, 0.0], [0.3, 0.4]], _ulp_above_case(),
     [("record, s2 == m2", 0, False), ("record 0.3 0.4", 1, None), ("body, s2 == m2", 2, False), ("body, s2 one ulp above", 3, True),
      ("body, vz alone == m", 4, False), ("body, vz and one ulp", 5, True)]),
    ("min_speed 0", 0.0, [[0.0, 0.0], [1e-30, 0.0], [-0.0, 1e-20]], [[0.0, 0.0, -0.0], [0.0, 0.0, 1e-19]],
     [("s2 == 0 is not > 0", 0, False), ("vx*vx underflows to 0", 1, False), ("1e-40, a subnormal s2", 2, True), ("body at rest", 3, False),
      ("body, subnormal s2", 4, True)]),
    ("velocities that are not finite", 0.05, [[np.nan, 1.0], [1.0, np.inf], [1e300, 0.0], [3e38, 3e38]],
     [[np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0], [0.0, 0.0, np.nan], [1.0, 1.0, -1e39], [2e19, 2e19, 2e19], [1.0, 2.0, 3.0]],
     [("record vx NaN", 0, False), ("record vy inf", 1, False), ("record vx inf as fp32", 2, False), ("finite, s2 overflows: a label", 3, True),
      ("body vx inf", 4, False), ("body vy -inf", 5, False), ("body vz NaN", 6, False), ("body vz -inf as fp32", 7, False),
      ("body finite, s2 overflows", 8, True), ("body", 9, True)]),
    ("no bodies, body codes present", 0.05, lf.REC[:, 6:8], np.zeros((0, 3)),
     [("record", 0, True), ("first body code", 3, False), ("a later one", 5, False), ("ground", -1, False)]),
    ("no records", 0.05, np.zeros((0, 2)), lf.BODY_VEL, [("code 0 is body 0", 0, True), ("code 2 is body 2, too slow", 2, False), ("code 3", 3, False)]),
    ("nothing at all", 0.0, np.zeros((0, 2)), np.zeros((0, 3)), [("code 0", 0, False), ("ground", -1, False)]),
]


def _label_hex(row):
    return " ".join(f"{int(b):08x}" for b in np.ascontiguousarray(row, f32).view(np.uint32))


@pytest.fixture(scope="module")
def expected():
    """(the program's input, the reading's answers line by line)"""
    lines, want = [], []
    for z in Z_ORDER:
        for code in (5, lf.HIT_NONE):
            lines.append(f"K {zbits(z)} {code}")
            key = lref.pack_key([z], [code])
            want.append(f"K {int(key[0]):016x} {int(lref.key_code(key)[0])}")
    for code in ROUND_TRIP_CODES:
        lines.append(f"K {zbits(1.25)} {code}")
        key = lref.pack_key([1.25], [code])
        assert int(lref.key_code(key)[0]) == code
        want.append(f"K {int(key[0]):016x} {code}")
    for _, pts, _ in WINNERS:
        lines.append(f"W {len(pts)} " + " ".join(f"{zbits(z)} {c}" for z, c in pts))
        key = lref.pack_key([z for z, _ in pts], [c for _, c in pts]).min()
        want.append(f"W {int(key):016x} {int(lref.key_code([key])[0])}")
    for _, m, rec, bodies, codes in SOURCES:
        rec, bodies = np.asarray(rec, np.float64).reshape(-1, 2), np.asarray(bodies, np.float64).reshape(-1, 3)
        lines.append(f"S {zbits(m)} {len(rec)} {len(bodies)} {hex64(rec)} {hex64(bodies)}")
        want.append(f"S {len(rec)} {len(bodies)}")
        for _, code, _ in codes:
            lines.append(f"L {code}")
            want.append("L " + _label_hex(lref.label_of([code], rec, bodies, m)[0]))
    return "\n".join(lines) + "\n", want


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "label_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "label_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "labels")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "labels_san")
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0:
        if "asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr:
            pytest.skip("the sanitizer runtime is not installed: " + build.stderr.strip().splitlines()[-1])
        raise AssertionError(build.stderr)
    return out


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
    kinds = {k: sum(1 for w in want if w.startswith(k)) for k in "KWSL"}
    print("lines per kind:", kinds)
    assert all(v >= len(SOURCES) for v in kinds.values())
    zero = "L " + _label_hex([0, 0, 0, 0])
    assert sum(1 for w in want if w == zero) > 10 and sum(1 for w in want if w.startswith("L") and w.endswith("3f800000")) > 10


def test_host_rules_equal_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_rules_run_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


# ---- 2. the cases do what they are named for ----------------------------------------------------------------------------
def test_the_keys_rise_from_negative_through_the_zeros_to_positive():
    z = np.array(Z_ORDER, f32)
    assert np.all(np.isfinite(z)) and np.all(np.diff(z[z != 0]) > 0) and np.signbit(z[6]) and not np.signbit(z[7])
    for code in (5, lf.HIT_NONE, INT_MAX, INT_MIN):
        key = lref.pack_key(z, np.full(len(z), code))
        assert np.all(key[1:] > key[:-1]) and key.max() < lref.KEY_EMPTY
    # the largest key a finite point can make stays below "empty"
    assert lref.pack_key([np.finfo(f32).max], [INT_MIN])[0] < lref.KEY_EMPTY
    assert lref.pack_key([np.finfo(f32).max], [INT_MIN])[0] >> np.uint64(32) == np.uint64(0xFF7FFFFF)


def test_the_winner_cases_are_won_as_named():
    for name, pts, winner in WINNERS:
        key = lref.pack_key([z for z, _ in pts], [c for _, c in pts]).min()
        assert int(lref.key_code([key])[0]) == winner, name
        best = pts[0]
        for p in pts[1:]:                           # and by the rule spoken directly
            if lref._before(f32(p[0]), p[1], f32(best[0]), best[1]):
                best = p
        assert best[1] == winner, name


def test_the_label_cases_are_labelled_as_named():
    for name, m, rec, bodies, codes in SOURCES:
        rec, bodies = np.asarray(rec, np.float64).reshape(-1, 2), np.asarray(bodies, np.float64).reshape(-1, 3)
        for what, code, on in codes:
            lab = lref.label_of([code], rec, bodies, m)[0]
            if on is None:
                continue
            assert (lab[3] == 1.0) == on and lab[3] in (0.0, 1.0), (name, what, lab)
            if not on:
                assert lab.tobytes() == np.zeros(4, f32).tobytes(), (name, what, lab)      # +0 in every component
            else:
                src = rec[code].tolist() + [0.0] if 0 <= code < len(rec) else bodies[code - len(rec)]
                assert lab[:3].tobytes() == np.asarray(src, np.float64).astype(f32).tobytes(), (name, what, lab)


# ---- 3. against a different algorithm -------------------------------------------------------------------------------------
def _random_cloud(seed, n):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.8, 1.8, n), np.round(rng.uniform(-0.2, 5.3, n) * 32) / 32], axis=1)
    xyz = xyz.astype(f32)
    xyz[rng.integers(0, n, n // 50), rng.integers(0, 3, n // 50)] = np.nan
    xyz[rng.integers(0, n, 20), 2] = -0.0
    code = rng.integers(-2, 9, n).astype(np.int32)
    return xyz, code


@pytest.mark.parametrize("seed,n,cap,leaf", [(1, 3000, 5000, 0.15), (2, 4001, 300, 0.15), (3, 2500, 5000, 0.4), (4, 1, 10, 0.15)])
def test_the_loop_over_a_dict_of_leaves_equals_the_vectorised_reading(seed, n, cap, leaf):
    xyz, code = _random_cloud(seed, n)
    rng = [f32(4.95), f32(4.95), f32(1.5)]
    args = (leaf, cap, rng, lf.REC[:, 6:8], lf.BODY_VEL, lf.MIN_SPEED)
    a, b = lref.filter_labelled(xyz, code, *args), lref.filter_labelled_loop(xyz, code, *args)
    assert a[3] == b[3] and a[3] == len(a[0]) <= cap
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    if n > 1000:
        assert (a[1][:, 3] == 1.0).sum() > 20 and (a[1][:, 3] == 0.0).sum() > 20 and len(set(a[2].tolist())) >= 8
        # ties between codes happened, and the larger one took them: no leaf's winner is SOGM_HIT_NONE unless it is alone
        full = lref.filter_labelled(xyz, code, leaf, 10 ** 6, [f32(1e9)] * 3, lf.REC[:, 6:8], lf.BODY_VEL, lf.MIN_SPEED)
        assert full[3] > a[3] or cap >= full[3]                  # isInRange or the cap dropped leaves
    if cap == 300:
        assert a[3] == cap
        more = lref.filter_labelled(xyz, code, leaf, 5000, *args[2:])
        assert all(x.tobytes() == y[:cap].tobytes() for x, y in zip(a[:3], more[:3]))


def test_too_many_leaves_and_no_points():
    far = np.array([[0.0, 0.0, 0.0], [30.0, 30.0, 30.0]], f32)
    for fn in (lref.filter_labelled, lref.filter_labelled_loop):
        out = fn(far, [0, 1], 0.15, 10, [f32(100.0)] * 3, lf.REC[:, 6:8], None, 0.0, max_cells=1 << 20)
        assert out[3] == -1 and len(out[0]) == len(out[1]) == len(out[2]) == 0
        out = fn(far, [0, 1], 0.15, 10, [f32(100.0)] * 3, lf.REC[:, 6:8], None, 0.0, max_cells=1 << 24)
        assert out[3] == 2 and out[2].tolist() == [0, 1]
        out = fn(np.full((3, 3), np.nan, f32), [0, 1, 2], 0.15, 10, [f32(100.0)] * 3, lf.REC[:, 6:8], None, 0.0)
        assert out[3] == 0


# ---- 4. the hand-built clouds ---------------------------------------------------------------------------------------------
def test_every_named_leaf_is_won_by_the_code_it_is_named_for():
    raw, code, rng, per, cases = lf.clouds()
    assert len(per[0][1]) % 64 != 0 and len(per[2][1]) % 64 != 0 and len(per[1][1]) == 0
    assert all(200 < len(p[1]) < 1000 for p in (per[0], per[2]))
    wide = [f32(1e9)] * 3
    pts, lab, codes, n = lref.filter_labelled(*per[0], lf.LEAF, 5000, wide, lf.REC[:, 6:8], lf.BODY_VEL, lf.MIN_SPEED)
    won = dict(zip(lf.leaf_of_output(pts), codes.tolist()))
    assert len(won) == n == len(cases)                                     # every leaf of agent 0 has a name
    for name, (leaf, winner) in cases.items():
        assert won[leaf] == winner, (name, leaf, won[leaf], winner)
    # with the map's range one leaf goes, and the ranks behind it shift
    pts_r, lab_r, codes_r, n_r = lref.filter_labelled(*per[0], lf.LEAF, 5000, [f32(4.95), f32(4.95), f32(1.5)], lf.REC[:, 6:8],
                                                     lf.BODY_VEL, lf.MIN_SPEED)
    gone = lf.leaf_of_output(pts).index(cases["a leaf dropped by isInRange"][0])
    assert n_r == n - 1 and 0 < gone < n - 1
    assert np.array_equal(codes_r, np.delete(codes, gone)) and lab_r.tobytes() == np.delete(lab, gone, axis=0).tobytes()
    # the long runs span waves as their names say: the run's first point's lane
    xyz = per[0][0]
    ijk = lref.leaf_ijk(xyz, lf.LEAF)
    for name, lane, length in (("a run of 160 from lane 0, the winner at its first lane", 0, 160),
                               ("a run of 160 from lane 32, the winner at the first wave's last lane", 32, 160),
                               ("a run of 150 from lane 0, the winner in the following wave", 0, 150),
                               ("a run of 70 across two waves, the winner its last point", 22, 70)):
        idx = np.nonzero((ijk == cases[name][0]).all(axis=1) & np.isfinite(xyz).all(axis=1))[0]
        assert len(idx) == length and idx[0] % 64 == lane and np.array_equal(idx, np.arange(idx[0], idx[0] + length)), name
    a_idx = np.nonzero((ijk == (0, 3, 12)).all(axis=1))[0]
    assert np.diff(a_idx).max() > 1                                         # A B A: two runs
