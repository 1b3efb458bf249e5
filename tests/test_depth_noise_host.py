"""CPU: the depth camera's sensor-noise pass (include/sogm_abi.h "sensor noise") without a GPU.
  1. the bodies of csrc/sogm_depthnoise.hpp, compiled with the host compiler (tests/depth_noise_rules_host_test.cpp), against
     the numpy reading of the header (tests/depth_noise_reference.py), bit for bit: the known answers, 2 * 10^5 draws, pixels
     named for their branch, every pixel of the rendered branch scene; the same program under -fsanitize=address,undefined
     runs them clean;
  2. the reading held to itself: what the named pixels are named for, the identity at all-zero parameters, the counter
     identity, a shard against the whole swarm, another seed or frame;
  3. the statistics of the definition, against bounds derived from the sample size."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_noise_fixtures as nf  # noqa: E402
import depth_noise_reference as nref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DRAWS = 200000


def hexes(v):
    return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(v, np.float64).reshape(-1).view(np.uint64))


def image_case(cam, prm, depth, hit=None):
    """(the program's input for one I case, the reading's answer line by line)"""
    depth = np.asarray(depth, np.uint16).reshape(-1, cam.rows, cam.cols)
    head = " ".join(["I", hexes([cam.fx, cam.fy, cam.cx, cam.cy, cam.max_depth, cam.depth_scale]), str(cam.rows), str(cam.cols),
                     f"{prm.seed:x} {prm.frame:x}", str(prm.agent_base),
                     hexes([prm.sigma0, prm.sigma1, prm.sigma2, prm.p_drop, prm.edge_jump, prm.p_edge, prm.min_depth]),
                     str(len(depth)), "1" if hit is not None else "0"])
    if hit is None:
        body = " ".join(f"{int(d):x}" for d in depth.reshape(-1))
    else:
        h32 = np.asarray(hit, np.int32).reshape(-1).view(np.uint32)
        body = " ".join(f"{int(d):x} {int(h):x}" for d, h in zip(depth.reshape(-1), h32))
    d, cloud, h, counts = nref.add_noise(cam, prm, depth, hit)
    want, n = [], cam.rows * cam.cols
    cl = cloud.view(np.uint32).reshape(len(depth), n, 3)
    for a in range(len(depth)):
        want.append("C " + " ".join(str(int(c)) for c in counts[a]))
        da = d[a].reshape(-1)
        ha = h[a].reshape(-1).view(np.uint32) if h is not None else None
        for i in range(n):
            line = f"P {int(da[i]):04x} {int(cl[a, i, 0]):08x} {int(cl[a, i, 1]):08x} {int(cl[a, i, 2]):08x}"
            want.append(line + (f" {int(ha[i]):08x}" if ha is not None else ""))
    return head + "\n" + body + "\n", want


@pytest.fixture(scope="module")
def expected():
    """(the program's input, the reading's answers line by line)"""
    lines, want = [], []
    for x in (0, 1, 0x5067, 2 ** 64 - 1):
        lines.append(f"M {x:x}\n")
        want.append(f"M {int(nref.mix(x)):016x}")
    # the header's known answers, literally
    assert want[0] == "M e220a8397b1dcdaf"
    lines.append("K 5067 3 0\n")
    want.append("K 52e3cb0b7bf29351 436624 " + hexes(float.fromhex("0x1.532cp-1")))
    h = nref.pixel_key(0x5067, 3, 0)
    assert int(h) == 0x52E3CB0B7BF29351 and int(nref.pieces_sum(h)) == 436624 and float(nref.normal(h)) == float.fromhex("0x1.532cp-1")
    lines.append(f"R 5067 3 0 {N_DRAWS}\n")
    hs = nref.pixel_key(0x5067, 3, np.arange(N_DRAWS, dtype=np.uint64))
    u0, u1, n = nref.uniform(nref.draw(hs, 0)), nref.uniform(nref.draw(hs, 1)), nref.normal(hs)
    want += [f"R {a:016x} {b:016x} {c:016x}" for a, b, c in zip(u0.view(np.uint64).tolist(), u1.view(np.uint64).tolist(),
                                                                  n.view(np.uint64).tolist())]
    for name, img, prm, _, _ in nf.named_pixels():
        text, w = image_case(nf.small_cam(*img.shape), prm, img)
        lines.append(text)
        want += w
    cam, depth, hit = nf.scene_frames(37, 53)
    text, w = image_case(cam, nf.active_params(), depth, hit)
    lines.append(text)
    want += w
    text, w = image_case(cam, nf.active_params(frame=4, agent_base=5), depth)       # without a hit image, another shard
    lines.append(text)
    want += w
    return "".join(lines), want


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "depth_noise_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "depth_noise_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "noise")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "noise_san")
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
    kinds = {k: sum(1 for w in want if w.startswith(k)) for k in ("M", "K", "R", "C", "P 0000", "P")}
    print("lines per kind:", kinds)
    assert kinds["R"] == N_DRAWS and kinds["P 0000"] > 1000 and kinds["P"] - kinds["P 0000"] > 5000


def test_host_rule_equals_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_rule_runs_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


# ---- 2. the reading held to itself ------------------------------------------------------------------------------------------
def test_the_named_pixels_do_what_they_are_named_for():
    for name, img, prm, (v, u), counter in nf.named_pixels():
        cam = nf.small_cam(*img.shape)
        out, counts, masks = nref.noise_image(cam, prm, 0, img)
        assert counts[0] == counts[1:].sum() == (img != 0).sum(), name
        if counter == "returns_out":
            assert masks.out[v, u] and out[v, u] != 0, name
        else:
            assert getattr(masks, counter)[v, u] and out[v, u] == 0, name
        if img.size == 1:
            assert counts[nref.COUNTERS.index(counter)] == 1 and counts[0] == 1, (name, counts)
    by = {name: (img, prm) for name, img, prm, _, _ in nf.named_pixels()}
    img, prm = by["returns_out: a noised return"]
    assert nref.noise_image(nf.small_cam(1, 1), prm, 0, img)[0][0, 0] not in (0, 2000)            # noised, not dropped
    for name, n_out in (("p_drop = 0 never drops", 64), ("p_drop = 1 always drops", 0), ("p_edge = 0 never drops", 32),
                        ("p_edge = 1 always drops", 0), ("corners and borders of a flat image are not edges", 9),
                        ("a corner beside a hole", 0), ("1 x N beside the hole", 2), ("N x 1 beside the hole", 2)):
        img, prm = by[name]
        assert nref.noise_image(nf.small_cam(*img.shape), prm, 0, img)[1][5] == n_out, name
    img, prm = by["q == 0 with min_depth == 0"]
    z, n = 0.001, float(nref.normal(nref.pixel_key(prm.seed, prm.frame, 0)))
    assert 0.0 <= z + prm.sigma0 * n < 0.0005 and prm.min_depth == 0.0                            # in range, rounds to 0
    img, prm = by["zn negative"]
    assert 0.1 + prm.sigma0 * n < 0.0


def test_the_branch_scene_takes_every_branch():
    cam, depth, hit = nf.scene_frames(37, 53)
    d, cloud, h, counts = nref.add_noise(cam, nf.active_params(), depth, hit)
    print("counts per camera:", counts.tolist())
    assert (counts.sum(axis=0) > 0).all()
    assert np.array_equal(counts[:, 0], counts[:, 1:].sum(axis=1))
    assert np.array_equal(counts[:, 0], (depth != 0).sum(axis=(1, 2))) and np.array_equal(counts[:, 5], (d != 0).sum(axis=(1, 2)))
    assert np.array_equal(h == nref.HIT_NONE, d == 0) and np.array_equal(h[d != 0], hit[d != 0])
    assert np.array_equal(np.isnan(cloud).any(axis=1), d.reshape(-1) == 0)
    assert ((d != depth) & (d != 0)).sum() > 1000                                                 # returns that moved


def test_all_zero_parameters_are_the_identity():
    """on every d16 a camera can give at depth_scale 1000 (65535 = max_depth * depth_scale at the most), and on the scene with
    its cloud and hit"""
    cam = nf.small_cam(1, 65535)
    cam.max_depth = 65.535
    img = np.arange(1, 65536, dtype=np.uint16).reshape(1, -1)
    out, counts, _ = nref.noise_image(cam, nref.params(nf.SEED, 9), 0, img)
    assert np.array_equal(out, img) and counts.tolist() == [65535, 0, 0, 0, 0, 65535]
    import body_fixtures as bf
    import depth_bodies_reference as bref
    rec, cam, pos, rot, bodies, _ = bf.branch_scene(37, 53)
    depth, cloud, _, hit = bref.render_agents(rec, cam, pos, rot, bodies, None, rings=True)
    d, cl, h, counts = nref.add_noise(cam, nref.params(nf.SEED, 9), depth, hit)
    assert np.array_equal(d, depth) and np.array_equal(h, hit) and nref.same_cloud(cl, cloud)
    assert np.array_equal(counts[:, 0], counts[:, 5]) and (counts[:, 1:5] == 0).all()


def test_a_shard_draws_what_the_whole_swarm_would():
    cam, depth, hit = nf.scene_frames(37, 53)
    full = nref.add_noise(cam, nf.active_params(), depth[:3], hit[:3])
    part = nref.add_noise(cam, nf.active_params(agent_base=1), depth[1:3], hit[1:3])
    n = cam.rows * cam.cols
    assert np.array_equal(part[0], full[0][1:3]) and np.array_equal(part[2], full[2][1:3])
    assert np.array_equal(part[3], full[3][1:3]) and nref.same_cloud(part[1], full[1][n:3 * n])


def test_another_seed_or_frame_gives_another_image():
    cam, depth, _ = nf.scene_frames(37, 53)
    base = nref.add_noise(cam, nf.active_params(), depth)[0]
    for other in (nf.active_params(frame=4), nf.active_params(seed=nf.SEED + 1)):
        d = nref.add_noise(cam, other, depth)[0]
        assert (d != base).mean() > 0.3
    assert np.array_equal(nref.add_noise(cam, nf.active_params(), depth)[0], base)


# ---- 3. the statistics of the definition ------------------------------------------------------------------------------------
def test_the_draws_have_the_statistics_the_header_states():
    """N draws of a unit-variance n: the mean has standard deviation 1/sqrt(N), the sample variance sqrt(2/N) (the fourth
    moment of a 12-piece Irwin-Hall sum is 2.9, below the normal's 3); a share of N Bernoulli(p) draws sqrt(p (1 - p)/N).
    Five standard deviations each."""
    N = N_DRAWS
    h = nref.pixel_key(0x5067, 3, np.arange(N, dtype=np.uint64))
    n = nref.normal(h)
    print(f"mean {n.mean():+.4f} var {n.var():.4f} min {n.min():+.3f} max {n.max():+.3f}")
    assert abs(n.mean()) <= 5.0 / np.sqrt(N)
    assert abs(n.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert round(float(n.mean()), 4) == -0.0047 and round(float(n.var()), 4) == 0.9972          # the header's figures
    assert np.abs(n).max() < 6.0
    for k, p in ((0, 0.05), (1, 0.5)):
        u = nref.uniform(nref.draw(h, k))
        assert (u >= 0).all() and (u < 1).all()
        share = (u < p).mean()
        print(f"share of U(w_{k}) < {p}: {share:.4f}")
        assert abs(share - p) <= 5.0 * np.sqrt(p * (1.0 - p) / N)
        if k == 0:
            assert round(float(share), 4) == 0.0508
