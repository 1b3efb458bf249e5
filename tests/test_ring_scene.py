"""CPU: rings in scene.make_scene / scene.WorldTimeline.  n_rings = 0 gives the scene and the frames that the code before
rings gave, byte for byte (digests recorded from that code for the seeds the suite uses); with rings every ring point's owner
indexes a type-2 record and frame(k) moves a ring's points and its record together."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import world_frames_reference as wref  # noqa: E402

# sha256 over make_scene's arrays (sorted keys) and WorldTimeline.frame(k), k = 0, 1, 37 (cloud, cylinders, their
# SogmCylinder bytes), computed with the scene module of the commit before rings
BEFORE = {
    (4, 0x5069): "23e492bb0e5864a92759e905126d1760099056246f06dcbbb8e9d672a7f04a9c",
    (4, 7): "c746d3140dd800aa0592ba5f8d51ae573dd42d6122e31d51cc651539563c3c20",
    (2, 0x5067): "44ddc229fb0a89af0ff8d7758152920c423cafb3462a57abd7af5126345a75b7",
    (8, 0x5069): "1d8958eb609d1c158fe543debc0c92a68ddeadad8d3e30f89a77fe32eeb89f95",
    (2, 7): "ea24e73880d724db1da46560373c39fb042ccd72f2e951d6c32ade11ec83711a",
}


def digest(scene_mod, n_agents, seed, **kw):
    sc = scene_mod.make_scene(n_agents, 4.95, seed=seed, **kw)
    h = hashlib.sha256()
    for k in sorted(sc):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sc[k]).tobytes())
    tl = scene_mod.WorldTimeline(sc, 0.1, moving=True)
    for k in (0, 1, 37):
        f = tl.frame(k)
        assert sorted(f) == ["cloud", "cylinders"]
        h.update(np.ascontiguousarray(f["cloud"]).tobytes())
        h.update(np.ascontiguousarray(f["cylinders"]).tobytes())
        h.update(bytes(scene_mod.cylinders_to_struct(f["cylinders"])))
    return h.hexdigest()


@pytest.mark.parametrize("key", sorted(BEFORE), ids=lambda k: f"{k[0]} agents, seed {k[1]:#x}")
def test_no_rings_is_the_scene_of_before(pop, key):
    assert digest(pop.scene, key[0], key[1]) == BEFORE[key]
    assert digest(pop.scene, key[0], key[1], n_rings=0) == BEFORE[key]


@pytest.fixture(scope="module")
def ringed(pop):
    return pop.scene.make_scene(4, 4.95, seed=0x5069), pop.scene.make_scene(4, 4.95, seed=0x5069, n_rings=5)


def test_rings_are_added_behind_everything_that_was_there(pop, ringed):
    sc0, sc = ringed
    n0 = len(sc0["cloud"])
    for k in sc0:
        if k not in ("cloud", "cloud_cyl"):
            assert np.array_equal(sc[k], sc0[k]), k
    assert np.array_equal(sc["cloud"][:n0], sc0["cloud"]) and np.array_equal(sc["cloud_cyl"][:n0], sc0["cloud_cyl"])
    assert sc["rings"].shape == (5, 10) and len(sc["cloud"]) > n0 + 5 * 9 * 8
    arr, n = pop.scene.records_to_struct(sc["cylinders"], sc["rings"])
    n_cyl = len(sc["cylinders"])
    assert n == n_cyl + 5 and bytes(arr)[:96 * n_cyl] == bytes(pop.scene.cylinders_to_struct(sc["cylinders"]))[:96 * n_cyl]
    own = sc["cloud_cyl"][n0:]
    assert set(own.tolist()) == set(range(n_cyl, n)) and all(arr[int(o)].type == 2 for o in set(own.tolist()))
    assert all(arr[i].type == 3 for i in range(n_cyl)) and all(arr[i].h == pop.scene.RING_TUBE for i in range(n_cyl, n))
    # upright and tilted, moving in xy, every point within the tube section's corner of its ring's circle
    normals = np.array([pop.scene._quat_to_matrix(r[6:] / np.linalg.norm(r[6:]))[:, 2] for r in sc["rings"]])
    assert (np.abs(normals[0::2, 2]) < 1e-12).all() and (np.abs(normals[1::2, 2]) > 1e-3).all()
    assert (np.hypot(sc["rings"][:, 4], sc["rings"][:, 5]) > 0).all()
    for i, r in enumerate(sc["rings"]):
        p = sc["cloud"][n0:][own == n_cyl + i].astype(np.float64) - r[:3]
        along = p @ normals[i]
        radial = np.linalg.norm(p - along[:, None] * normals[i][None, :], axis=1)
        assert np.abs(along).max() < 0.1 + 1e-5 and np.abs(radial - 0.5 * r[3]).max() < 0.1 + 1e-5


@pytest.mark.parametrize("k", [0, 1, 37])
def test_a_frame_moves_a_ring_and_its_points_together(pop, ringed, k):
    """frame(k) against the world timeline's second reading (tests/world_frames_reference.py), which is type-agnostic: the
    rings' rows appended to the cylinders' as records"""
    _, sc = ringed
    tl = pop.scene.WorldTimeline(sc, 0.1, moving=True)
    arr0, n = tl.records(0)
    rows0 = np.array([[o.x, o.y, o.z, o.w, o.h, o.vx, o.vy, o.qw, o.qx, o.qy, o.qz] for o in arr0][:n])
    cloud, _, rows = wref.frame(sc["cloud"], sc["cloud_cyl"], rows0, 0.1, 1, k)
    f = tl.frame(k)
    assert np.array_equal(cloud.view(np.uint32), np.ascontiguousarray(f["cloud"], np.float32).view(np.uint32))
    arr, _ = tl.records(k)
    got = np.array([[o.x, o.y, o.z, o.w, o.h, o.vx, o.vy, o.qw, o.qx, o.qy, o.qz] for o in arr][:n])
    assert np.array_equal(got.view(np.uint64), rows.view(np.uint64))
    assert [o.type for o in arr][:n] == [3] * len(sc["cylinders"]) + [2] * 5
    if k:
        n_cyl = len(sc["cylinders"])
        ring_pts = sc["cloud_cyl"] >= n_cyl
        moved = f["cloud"][ring_pts, :2] - sc["cloud"][ring_pts, :2]
        want = (sc["rings"][:, 4:6] * (k * 0.1))[sc["cloud_cyl"][ring_pts] - n_cyl]
        assert np.abs(moved - want).max() < 1e-5 and np.abs(f["rings"][:, :2] - sc["rings"][:, :2] - sc["rings"][:, 4:6] * (k * 0.1)).max() < 1e-12
        assert np.array_equal(f["cloud"][ring_pts, 2], sc["cloud"][ring_pts, 2]) and np.array_equal(f["rings"][:, 2:], sc["rings"][:, 2:])


def test_a_frozen_timeline_keeps_the_rings_where_they_are(pop, ringed):
    _, sc = ringed
    tl = pop.scene.WorldTimeline(sc, 0.1, moving=False)
    assert np.array_equal(tl.frame(9)["rings"], sc["rings"]) and tl.frame(9)["cloud"] is tl.cloud0
