"""GPU: sogm_world_frames (include/sogm_abi.h "world timeline") — the kernel of csrc/sogm_world.hip against the numpy
reading of the header (tests/world_frames_reference.py), bit for bit: the cloud as int32, the records as bytes, the bounds
against the reading AND against sogm_cloud_block_bounds run on the uploaded reference cloud.  Every output buffer carries
64 guard bytes behind it (and the offset in front of it, where it has one) that must come back untouched: the tails of the
16-byte stores.  Then the driver: SwarmTick on device frames from the smallest pool flies the same records as on uploaded
frames."""
import ctypes as C
import importlib

import numpy as np
import pytest

import world_frames_reference as ref

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
N_POINTS = [1, 63, 64, 65, 257, 1000, 4097]
BLOCK_POINTS = [64, 256, 4096]
TYPES, PADS = np.array([3, 2, 3, 7, 3]), np.array([0, -5, 0x1234, 0, 9])


def _sogm():
    return importlib.import_module("pred-occ-planner_amd.sogm")


class Guarded:
    """nbytes of device memory at `offset` bytes into an allocation, FILL in front of and behind it"""

    def __init__(self, nbytes, offset=0, data=None):
        import torch
        self.nbytes, self.offset = int(nbytes), int(offset)
        self.t = torch.full((self.offset + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert len(raw) == self.nbytes
            if self.nbytes:
                self.t[self.offset:self.offset + self.nbytes] = torch.from_numpy(raw.copy()).cuda()
        self.ptr = self.t.data_ptr() + self.offset

    def read(self, dtype):
        h = self.t.cpu().numpy()
        assert (h[:self.offset] == FILL).all() and (h[self.offset + self.nbytes:] == FILL).all(), "guard bytes were written"
        return h[self.offset:self.offset + self.nbytes].copy().view(dtype)


def make_world(n_points, n_cyl, seed):
    rng = np.random.RandomState(seed)
    cloud = rng.uniform(-30, 30, (n_points, 3)).astype(np.float32)
    owner = ((np.arange(n_points) // 21) % max(n_cyl, 1)).astype(np.int32)   # a block of 64 spans four owners
    owner[5::17], owner[11::19] = -1, n_cyl                                  # static points: below and above the range
    rows = np.zeros((n_cyl, 11), np.float64)
    rows[:, 0:2] = rng.uniform(-30, 30, (n_cyl, 2))
    rows[:, 2], rows[:, 4], rows[:, 7] = 2.0, 4.0, 1.0
    rows[:, 3] = rng.uniform(0.5, 1.0, n_cyl)
    rows[:, 5:7] = rng.uniform(-1, 1, (n_cyl, 2))
    if n_cyl > 2:
        rows[2, 5:7] = 0.0                                                   # a record that stands still ...
        if n_points > 45:
            assert owner[45] == 2
            cloud[45] = (-0.0, -0.0, -0.0)                                   # ... and a -0.0f point of its own
    return cloud, owner, rows


def run_frames(pop, cloud0, owner, rows, dt, moving, first_tick, n_ticks, block_points, in_off=0, out_off=0):
    """the call on guarded buffers -> [(cloud float32 [n, 3], bounds float32 [nb, 4], records uint8)] per tick"""
    import torch
    abi = pop._abi
    n, n_cyl = len(cloud0), len(rows)
    nb = -(-n // block_points)
    d_cloud0 = Guarded(n * 12, in_off, cloud0)
    d_owner = Guarded(n * 4, 0, owner.astype(np.int32))
    d_cyl0 = Guarded(n_cyl * 96, 0, ref.records_bytes(rows, TYPES[:n_cyl], PADS[:n_cyl]))
    tl = abi.SogmWorldTimeline(d_cloud0.ptr if n else None, d_owner.ptr if n else None, d_cyl0.ptr if n_cyl else None, n, n_cyl,
                               block_points, moving, dt)
    outs = [(Guarded(n * 12, out_off), Guarded(nb * 16), Guarded(n_cyl * 96)) for _ in range(n_ticks)]
    arr = (abi.SogmWorld * n_ticks)(*[abi.SogmWorld(c.ptr if n else None, b.ptr if n else None, r.ptr if n_cyl else None, n,
                                                    nb, block_points, n_cyl) for c, b, r in outs])
    abi.check(pop.lib().sogm_world_frames(C.byref(tl), first_tick, n_ticks, arr, _sogm()._stream()), "sogm_world_frames")
    torch.cuda.synchronize()
    for g in (d_cloud0, d_owner, d_cyl0):
        g.read(np.uint8)                  # the inputs' guards
    return [(c.read(np.float32).reshape(-1, 3), b.read(np.float32).reshape(-1, 4), r.read(np.uint8)) for c, b, r in outs]


def device_block_bounds(pop, cloud, block_points):
    import torch
    n, nb = len(cloud), -(-len(cloud) // block_points)
    d_cloud, d_out = Guarded(n * 12, 0, cloud), Guarded(nb * 16)
    if n:
        pop._abi.check(pop.lib().sogm_cloud_block_bounds(d_cloud.ptr, n, block_points, d_out.ptr, _sogm()._stream()),
                       "sogm_cloud_block_bounds")
    torch.cuda.synchronize()
    return d_out.read(np.float32).reshape(-1, 4)


def check_frames(pop, cloud0, owner, rows, dt, moving, first_tick, n_ticks, block_points, **kw):
    got = run_frames(pop, cloud0, owner, rows, dt, moving, first_tick, n_ticks, block_points, **kw)
    for i, (cloud, bounds, recs) in enumerate(got):
        k = first_tick + i
        w_cloud, w_bounds, w_rows = ref.frame(cloud0, owner, rows, dt, moving, k, block_points)
        tag = (len(cloud0), block_points, k, kw)
        assert np.array_equal(cloud.view(np.int32), w_cloud.view(np.int32)), tag
        assert np.array_equal(recs, ref.records_bytes(w_rows, TYPES[:len(rows)], PADS[:len(rows)])), tag
        assert np.array_equal(bounds.view(np.int32), w_bounds.view(np.int32)), tag
        assert np.array_equal(bounds.view(np.int32), device_block_bounds(pop, w_cloud, block_points).view(np.int32)), tag
    return got


@pytest.mark.parametrize("block_points", BLOCK_POINTS)
@pytest.mark.parametrize("n_points", N_POINTS)
def test_kernel_equals_the_second_reading(pop, n_points, block_points):
    cloud0, owner, rows = make_world(n_points, 5, seed=n_points * 7 + block_points)
    if n_points >= 64:
        assert len(set(owner[:64].tolist())) >= 3       # a block that spans three owners (and static points)
    check_frames(pop, cloud0, owner, rows, 0.1, 1, 0, 1, block_points)
    got = check_frames(pop, cloud0, owner, rows, 0.1, 1, 36, 2, block_points)
    assert n_points < 64 or (got[0][0] != cloud0).any()
    if n_points > 45:   # the -0.0f point of the record that stands still: +0.0f once the add is performed, z copied
        assert (got[0][0][45].view(np.uint32) == [0, 0, 0x80000000]).all()


@pytest.mark.parametrize("block_points,in_off,out_off", [(65, 0, 0), (257, 0, 0), (4095, 0, 0), (64, 4, 4), (256, 8, 8),
                                                         (65, 12, 12), (64, 0, 4), (256, 8, 0)])
def test_blocks_and_buffers_off_the_16_byte_boundaries(pop, block_points, in_off, out_off):
    """block_points * 12 no multiple of 16 (blocks start off a boundary), buffers that start off one, and an input and an
    output that are not equally aligned (no 16-byte access at all)"""
    cloud0, owner, rows = make_world(1000, 5, seed=block_points + in_off)
    check_frames(pop, cloud0, owner, rows, 0.1, 1, 3, 2, block_points, in_off=in_off, out_off=out_off)


def test_a_frozen_world_and_tick_zero_are_copies(pop):
    cloud0, owner, rows = make_world(1000, 5, seed=11)
    for moving, first in ((0, 7), (1, 0)):
        got = check_frames(pop, cloud0, owner, rows, 0.1, moving, first, 1, 256)
        assert np.array_equal(got[0][0].view(np.int32), cloud0.view(np.int32))
        assert (got[0][0][45].view(np.uint32) == 0x80000000).all()


def test_no_records_and_records_only(pop):
    cloud0, owner, _ = make_world(1000, 5, seed=12)
    got = check_frames(pop, cloud0, owner, np.zeros((0, 11)), 0.1, 1, 4, 2, 256)      # n_cyl = 0: every point is static
    assert np.array_equal(got[1][0].view(np.int32), cloud0.view(np.int32))
    _, _, rows = make_world(0, 5, seed=13)
    got = check_frames(pop, np.zeros((0, 3), np.float32), np.zeros(0, np.int32), rows, 0.1, 1, 4, 2, 256)  # n_points = 0
    assert len(got[0][2]) == 5 * 96 and (got[0][2] != got[1][2]).any()
    big = np.zeros((300, 11))                                                         # more records than one workgroup's lanes
    big[:, 0:2] = np.arange(600).reshape(300, 2)
    big[:, 5:7] = 0.25
    abi = pop._abi
    types, pads = np.full(300, 3), np.zeros(300, np.int64)
    n_cyl = 300
    d_cyl0 = Guarded(n_cyl * 96, 0, ref.records_bytes(big, types, pads))
    out = Guarded(n_cyl * 96)
    tl = abi.SogmWorldTimeline(None, None, d_cyl0.ptr, 0, n_cyl, 256, 1, 0.1)
    arr = (abi.SogmWorld * 1)(abi.SogmWorld(None, None, out.ptr, 0, 0, 256, n_cyl))
    abi.check(pop.lib().sogm_world_frames(C.byref(tl), 9, 1, arr, None), "sogm_world_frames")
    import torch
    torch.cuda.synchronize()
    want = ref.frame(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), big, 0.1, 1, 9)[2]
    assert np.array_equal(out.read(np.uint8), ref.records_bytes(want, types, pads))


def test_one_call_for_seven_ticks_equals_seven_calls(pop):
    cloud0, owner, rows = make_world(4097, 5, seed=14)
    batch = run_frames(pop, cloud0, owner, rows, 0.1, 1, 5, 7, 256)
    for i in range(7):
        single = run_frames(pop, cloud0, owner, rows, 0.1, 1, 5 + i, 1, 256)[0]
        for a, b in zip(batch[i], single):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), i
    assert (batch[0][0] != batch[6][0]).any()


def test_world_timeline_dev_serves_world_compatible_frames_from_a_pool(pop):
    """sogm.WorldTimelineDev: frames of make_scene's world equal sogm.World built from scene.WorldTimeline's frame of the
    same tick, attribute by attribute; the pool's slots are taken in turn"""
    import torch
    sogm = _sogm()
    sc = pop.scene.make_scene(4, 4.95, seed=0x5069, moving=True)
    tl = pop.scene.WorldTimeline(sc, 0.1, moving=True)
    dev = sogm.WorldTimelineDev.from_timeline(tl, pool=3)
    a = dev.frames(4, 2)
    b = dev.frames(6, 2)
    assert b[1] is a[0] and b[0] is not a[1] and dev.pool == 3 and [f.tick for f in b] == [6, 7]
    with pytest.raises(ValueError):
        dev.frames(0, 4)
    for f in b:
        h = tl.frame(f.tick)
        w = sogm.World(h["cloud"], h["cylinders"])
        torch.cuda.synchronize()
        assert (f.n_points, f.n_blocks, f.block_points, f.n_cyl) == (w.n_points, w.n_blocks, w.block_points, w.n_cyl)
        assert (f.c.n_points, f.c.n_blocks, f.c.block_points, f.c.n_cyl) == (w.n_points, w.n_blocks, w.block_points, w.n_cyl)
        assert f.c.cloud_xyz == f.cloud.data_ptr() and f.c.block_bounds == f.bounds.data_ptr()
        assert torch.equal(f.cloud.view(torch.int32), w.cloud.view(torch.int32))
        assert torch.equal(f.bounds.view(torch.int32), w.bounds.view(torch.int32))
        assert torch.equal(f.cylinders, w.cylinders)


# ---- the driver on device frames ---------------------------------------------------------------------------------------
def _fly_steps(pop, device_world, **kw):
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    sw = driver.SwarmTick("parity", 4, moving_world=True, device_world=device_world, world_pool=2, **kw)
    assert sw.compute.device_world == device_world
    out = []
    for _ in range(6):
        ok = sw.step()
        out.append((ok.cpu().numpy().copy(), sw.own.cpu().numpy().copy(), sw.status.cpu().numpy().copy()))
    torch.cuda.synchronize()
    if device_world:    # no frame was uploaded, and six ticks came out of two slots
        assert not sw.compute._frames and sw.compute._tl_dev.pool == 2
    else:
        assert len(sw.compute._frames) == 6 and sw.compute._tl_dev is None
    sw.close()
    return out


@pytest.mark.parametrize("kw", [dict(prestamp=False), dict(prestamp=False, fsm=True, device_fsm=True),
                                dict(prestamp=True, grids=3), dict(prestamp=False, tuning={"update_flow": 1})],
                         ids=["step", "fsm on the device", "pre-stamp", "update flow"])
def test_step_on_device_frames_flies_the_same_records(pop, kw):
    """parity grid (66 x 66 x 20 x 6), 4 agents, moving world, 6 step() ticks: byte-identical records and ok flags, the pool
    at the smallest size the stream-order argument allows for lock-step ticks (2: sogm.WorldTimelineDev) — also with the
    two consumers that go on reading a frame on streams of their own, the pre-stamp and the update flow"""
    want, got = _fly_steps(pop, False, **kw), _fly_steps(pop, True, **kw)
    for k, (w, g) in enumerate(zip(want, got)):
        for a, b in zip(w, g):
            assert np.array_equal(a, b), (kw, k)
    assert sum(int(w[0].sum()) for w in want) >= 4    # replans did succeed


def test_fly_on_device_frames_flies_the_same_records(pop):
    """fly(4): the four frames of the flight from ONE batched call, a pool of exactly the flight in the air"""
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    res = []
    for dw in (False, True):
        sw = driver.SwarmTick("parity", 4, moving_world=True, prestamp=False, device_world=dw, world_pool=2)
        ok, rec = sw.fly(4)
        ok2, rec2 = sw.fly(4)     # the second flight rewrites the first one's slots
        torch.cuda.synchronize()
        assert sw.planner.flow_failures() == (0, 0)
        res.append([t.cpu().numpy().copy() for t in (ok, rec, ok2, rec2, sw.own)])
        if dw:
            assert not sw.compute._frames and sw.compute._tl_dev.pool == 4
        sw.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert int(res[0][0].sum()) >= 4
