"""GPU: sogm_view_mask and sogm_map_audit_masked against the numpy reading of "view mask" (tests/view_mask_reference.py).
  - the mask's words and the counts, bit for bit, on the hand-built batches of tests/test_view_mask_host.py (checked there, on
    the CPU, to make every class non-empty): each single class, FREE | SURFACE and all; agents with different rotations,
    images and offsets; out_counts NULL; guard words on both sides of the mask;
  - the two equivalences that tie the new entries to sogm_map_audit: every class but OUTSIDE is the frustum's region (r = 0,
    r = 2, a box), a mask of every live bit is the whole grid;
  - sogm_map_audit_masked against audit_with_region on random grids and the visible mask: r = 0 and 3, slab_layers 1 and 0,
    fp16 tiles against fp32 rows, a slice_map with a skipped slice, one agent's centre one ulp off;
  - both entries twice: identical bytes, nothing else written; every refusal, with nothing written;
  - the chain render_depth -> view_mask -> audit_against(mask=...) on a one-cylinder world, and the C++ facade."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_audit_reference as mref  # noqa: E402
import ring_fixtures as fx  # noqa: E402
import view_mask_reference as vref  # noqa: E402
from test_map_audit_gpu import F16, F32, ROW, TILED, Side  # noqa: E402
from test_view_mask_host import BAD_PRM, COLS, ROWS, batches, build_facade_program, good_prm, reading  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A5A5A5A5A
VISIBLE = vref.BIT[vref.FREE] | vref.BIT[vref.SURFACE]
IN_FRUSTUM = vref.ALL & ~vref.BIT[vref.OUTSIDE]


def _mods():
    return importlib.import_module("pred-occ-planner_amd"), importlib.import_module("pred-occ-planner_amd.sogm")


class VSide(Side):
    """test_map_audit_gpu.Side with a resolution of its own"""

    def __init__(self, dims, T, A, storage, res=0.15):
        pop, sogm = _mods()
        self.dims, self.T, self.A = dims, T, A
        self.V = dims[0] * dims[1] * dims[2]
        spec = pop.config.make_spec((*dims, T), map_kind=pop._abi.SOGM_MAP_FAKE, storage=storage)
        spec.resolution = float(res)
        self.m = sogm.SogmMap(spec, A)
        self.grids = None


def view_prm(prm, classes):
    pop, _ = _mods()
    p = pop._abi.SogmViewParams()
    for k, v in prm.items():
        setattr(p, k, v)
    p.classes = classes
    return p


def dev_mask(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def device_view(m, batch, classes):
    """(words uint64 [n, H, W, nw], counts int32 [n, 8]) of SogmMap.view_mask on a batch"""
    dims, res, prm, depths, rots, offs = batch
    mask, counts = m.view_mask(depths, view_prm(prm, classes), rots, cam_offset=offs)
    return mask.cpu().numpy().view(np.uint64), counts.cpu().numpy()


@pytest.fixture(scope="module")
def view_maps():
    """one context per (dims, resolution, agents) of the batches: only its geometry is used, it is never updated"""
    maps = {}

    def get(batch):
        dims, res, _, depths, _, _ = batch
        key = (dims, res, len(depths))
        if key not in maps:
            maps[key] = VSide(dims, 2, len(depths), F32, res)
        return maps[key].m

    yield get
    for s in maps.values():
        s.close()


# ---- sogm_view_mask against the reading ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(batches()))
def test_view_mask_equals_the_reading(view_maps, name):
    batch = batches()[name]
    m = view_maps(batch)
    for classes in [1 << c for c in range(5)] + [VISIBLE, vref.ALL]:
        cls, words, counts = reading(batch, classes)
        got_w, got_n = device_view(m, batch, classes)
        bad = np.argwhere(got_w != words)
        assert not len(bad), (name, classes, bad[:4].tolist(), hex(int(got_w[tuple(bad[0])])), hex(int(words[tuple(bad[0])])))
        assert np.array_equal(got_n, counts), (name, classes, got_n.tolist(), counts.tolist())
    print(name, "counts", counts[:, :6].tolist())
    assert (counts[:, :5].sum(axis=0) > 0).all()


def test_counts_null_guards_and_repeats(view_maps):
    """out_counts NULL; the words before and after [n][H][W][row_words] keep a guard pattern; twice the same bytes; the image,
    cam_rot and cam_offset are only read"""
    import torch
    pop, sogm = _mods()
    lib = pop.lib()
    batch = batches()["offset"]
    dims, res, prm, depths, rots, offs = batch
    m = view_maps(batch)
    _, words, counts = reading(batch, VISIBLE)
    n = words.size
    p = view_prm(prm, VISIBLE)
    img = torch.from_numpy(depths.view(np.int16)).cuda()
    rot, off = sogm._dev(rots, np.float64), sogm._dev(offs, np.float64)
    outs = []
    for with_counts in (False, True, True):
        buf = torch.full((n + 16,), GUARD, dtype=torch.int64, device="cuda")
        cnt = torch.full((len(depths) * 8 + 8,), -77, dtype=torch.int32, device="cuda")
        rc = lib.sogm_view_mask(m.ctx, C.byref(p), img.data_ptr(), rot.data_ptr(), off.data_ptr(), buf.data_ptr() + 64,
                                cnt.data_ptr() + 16 if with_counts else None, sogm._stream())
        assert rc == 0, lib.sogm_last_error()
        torch.cuda.synchronize()
        b, c = buf.cpu().numpy(), cnt.cpu().numpy()
        assert (b[:8] == GUARD).all() and (b[-8:] == GUARD).all() and np.array_equal(b[8:-8].view(np.uint64), words.reshape(-1))
        if with_counts:
            assert (c[:4] == -77).all() and (c[-4:] == -77).all() and np.array_equal(c[4:-4].reshape(-1, 8), counts)
        else:
            assert (c == -77).all()
        outs.append((b.tobytes(), c.tobytes()))
    assert outs[1] == outs[2]
    assert np.array_equal(img.cpu().numpy().view(np.uint16), depths) and np.array_equal(rot.cpu().numpy(), rots)
    assert np.array_equal(off.cpu().numpy(), offs)


# ---- the audit on a mask -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube_sides():
    """16^3, T = 2, three agents: fp16 tiles against fp32 rows, random grids"""
    dims = (16, 16, 16)
    test, truth = VSide(dims, 2, 3, F16 | TILED), VSide(dims, 2, 3, F32)
    rng = np.random.default_rng(0x766d)
    shape = (3, test.V, 2)
    test.put(values=np.where(rng.random(shape) < 0.3, rng.random(shape) + 0.21, rng.random(shape) * 0.2).astype(np.float32))
    truth.put(values=np.where(rng.random(shape) < 0.3, 1.0, 0.0).astype(np.float32))
    yield test, truth
    test.close()
    truth.close()


@pytest.fixture(scope="module")
def long_sides():
    """70 x 5 x 6 at 0.5 m, T = 3, three agents, fp32 rows (W is odd: no tiles)"""
    dims = (70, 5, 6)
    test, truth = VSide(dims, 3, 3, F32, 0.5), VSide(dims, 3, 3, F32, 0.5)
    rng = np.random.default_rng(0x6c6f)
    test.put(values=(rng.random((3, test.V, 3)) < 0.3).astype(np.float32))
    truth.put(values=(rng.random((3, test.V, 3)) < 0.3).astype(np.float32))
    yield test, truth
    test.close()
    truth.close()


def masked_rows(test, truth, mask, thr=(0.2, 0.2), r=0, box=None, slice_map=None, slab_layers=0):
    got = test.m.audit_against(truth.m, thr[0], thr[1], r, box, None, None, slice_map, slab_layers, mask=mask)
    assert np.array_equal(got["dt"], test.stamps - truth.stamps)
    return ROW(got)


def reading_rows(test, truth, R, thr=(0.2, 0.2), r=0, box=None, slice_map=None):
    return np.stack([vref.audit_with_region(test.grids[a], truth.grids[a], R[a], test.dims, thr[0], thr[1], r, box, slice_map,
                                            test.centres[a].tobytes() != truth.centres[a].tobytes()) for a in range(test.A)])


@pytest.mark.parametrize("r,box", [(0, None), (2, None), (1, ((1, 2, 3), (15, 16, 13)))], ids=["r0", "r2", "box"])
def test_every_class_but_outside_is_the_frustum_audit(cube_sides, r, box):
    """classes = OFFIMAGE | FREE | SURFACE | HIDDEN through sogm_map_audit_masked gives sogm_map_audit's rows with
    SOGM_MAPAUDIT_FRUSTUM and the same frustum, field for field (no cam_offset: the camera at the map centre)"""
    test, truth = cube_sides
    dims, res, prm, depths, rots, _ = batches()["cube"]
    mask, counts = test.m.view_mask(depths, view_prm(prm, IN_FRUSTUM), rots)
    got = masked_rows(test, truth, mask, r=r, box=box)
    fr = (prm["near_z"], prm["far_z"], prm["tan_h"], prm["tan_v"])
    want = ROW(test.m.audit_against(truth.m, 0.2, 0.2, r, box, fr, rots))
    assert np.array_equal(got, want), (got[0].tolist(), want[0].tolist())
    n = counts.cpu().numpy()
    if box is None:
        assert np.array_equal(got[:, 0, 0], n[:, 5]) and np.array_equal(n[:, 5], test.V - n[:, 0])
    assert got[0, 0, 0] > 0 and got[1, 0, 0] > 0 and got[2, 0, 0] == 0          # the NaN rotation sees nothing
    assert got[:2, :, 1].min() > 0 and got[:2, :, 2].min() > 0


@pytest.mark.parametrize("which", ["cube", "long"])
def test_a_mask_of_every_live_bit_is_the_whole_grid(cube_sides, long_sides, which):
    test, truth = cube_sides if which == "cube" else long_sides
    L, W, H = test.dims
    ones = np.ones((test.A, H, W, L), bool)
    full = np.stack([vref.pack(o) for o in ones])
    for r in (0, 1):
        want = ROW(test.m.audit_against(truth.m, 0.2, 0.2, r))
        assert np.array_equal(masked_rows(test, truth, dev_mask(full), r=r), want)
        # spare bits set in the mask are not cells: the rows do not change
        assert np.array_equal(masked_rows(test, truth, dev_mask(np.full_like(full, np.uint64(2 ** 64 - 1))), r=r), want)
    assert (want[:, :, 0] == test.V).all()


@pytest.mark.parametrize("which", ["cube", "long"])
def test_masked_audit_equals_the_reading_on_the_visible_mask(cube_sides, long_sides, which):
    test, truth = cube_sides if which == "cube" else long_sides
    batch = batches()["cube" if which == "cube" else "perms band 0.25"]
    dims, res, prm, depths, rots, offs = batch
    cls, words, counts = reading(batch, VISIBLE)
    R = (cls == vref.FREE) | (cls == vref.SURFACE)
    mask, _ = test.m.view_mask(depths, view_prm(prm, VISIBLE), rots, cam_offset=offs)
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), words)
    T = test.T
    skip = [T - 1] + [-1] * (T - 1) if T == 2 else [2, -1, 0]
    for r in (0, 3):
        want = reading_rows(test, truth, R, r=r)
        assert want[:, :, 4].sum() > 0 and want[:, :, 5].sum() > 0 and want[0, 0, 4] > 0 and want[0, 0, 5] > 0
        rows = [masked_rows(test, truth, mask, r=r, slab_layers=s) for s in (1, 0)]
        assert np.array_equal(rows[0], want), (r, rows[0][0].tolist(), want[0].tolist())
        assert np.array_equal(rows[1], want)
        print(which, "r", r, "agent 0 slice 0", want[0, 0, :6].tolist())
    box = ((1, 0, 1), (dims[0] - 2, dims[1], dims[2] - 1))
    assert np.array_equal(masked_rows(test, truth, mask, r=1, box=box, slice_map=skip, slab_layers=2),
                          reading_rows(test, truth, R, r=1, box=box, slice_map=skip))
    want = reading_rows(test, truth, R, r=1, slice_map=skip)
    assert (want[:, 1, 7] == mref.SKIPPED).all() and not want[:, 1, :6].any()
    assert np.array_equal(masked_rows(test, truth, mask, r=1, slice_map=skip), want)


def test_a_centre_one_ulp_off_is_that_agents_alone(cube_sides):
    test, truth = cube_sides
    batch = batches()["cube"]
    dims, res, prm, depths, rots, offs = batch
    cls = reading(batch, VISIBLE)[0]
    R = (cls == vref.FREE) | (cls == vref.SURFACE)
    mask, _ = test.m.view_mask(depths, view_prm(prm, VISIBLE), rots, cam_offset=offs)
    keep_t, keep_g = [g.copy() for g in test.grids], [g.copy() for g in truth.grids]
    c = np.array([[1.5, -2.25, 1.0], [0.3, 0.3, 0.9], [-4.0, 2.0, 1.0]], np.float32)
    d = c.copy()
    d[1, 2] = np.nextafter(d[1, 2], np.float32(2))
    try:
        test.put(values=np.stack(keep_t), centres=c)
        truth.put(values=np.stack(keep_g), centres=d)
        rows = masked_rows(test, truth, mask, r=1)
        assert np.array_equal(rows, reading_rows(test, truth, R, r=1))
        assert (rows[1, :, 7] == mref.CENTRE).all() and not rows[1, :, :6].any()
        assert (rows[0, :, 7] == 0).all() and rows[0, 0, 0] == R[0].sum() > 0 and (rows[2, :, 7] == 0).all()
    finally:
        test.put(values=np.stack(keep_t))
        truth.put(values=np.stack(keep_g))


def test_the_masked_audit_writes_nothing_and_repeats_itself(cube_sides):
    import torch
    test, truth = cube_sides
    batch = batches()["cube"]
    dims, res, prm, depths, rots, offs = batch
    mask, _ = test.m.view_mask(depths, view_prm(prm, VISIBLE), rots, cam_offset=offs)
    before = mask.cpu().numpy().copy()
    a = test.m.audit_against_device(truth.m, 0.2, 0.2, 2, mask=mask)
    b = test.m.audit_against_device(truth.m, 0.2, 0.2, 2, mask=mask)
    torch.cuda.synchronize()
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    assert np.array_equal(mask.cpu().numpy(), before)
    for s in (test, truth):
        assert all(np.array_equal(s.m.download(k), s.grids[k]) for k in range(s.A))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_view_mask(view_maps):
    import torch
    pop, sogm = _mods()
    lib, bad = pop.lib(), pop._abi.SOGM_ERR_INVALID_ARG
    batch = batches()["cube"]
    dims, res, prm, depths, rots, offs = batch
    m = view_maps(batch)
    img = torch.from_numpy(depths.view(np.int16)).cuda()
    rot, off = sogm._dev(rots, np.float64), sogm._dev(offs, np.float64)
    out = torch.full((3 * 16 * 16,), GUARD, dtype=torch.int64, device="cuda")
    cnt = torch.full((24,), -77, dtype=torch.int32, device="cuda")

    def rc(p=None, ctx=m.ctx, d=img.data_ptr(), r=rot.data_ptr(), o=out.data_ptr(), null_prm=False):
        p = good_prm(pop) if p is None else p
        return lib.sogm_view_mask(ctx, None if null_prm else C.byref(p), d, r, off.data_ptr(), o, cnt.data_ptr(), sogm._stream())

    refused = {"null map": rc(ctx=None), "null prm": rc(null_prm=True), "null depth": rc(d=None), "null cam_rot": rc(r=None),
               "null out_mask": rc(o=None), "2^32 pixels": rc(good_prm(pop, rows=65536, cols=65536))}
    for field, v in BAD_PRM:
        refused[f"{field} = {v}"] = rc(good_prm(pop, **{field: v}))
        assert lib.sogm_last_error().startswith(b"sogm_view_mask: ") and len(lib.sogm_last_error()) > 20, (field, v)
    assert all(v == bad for v in refused.values()), {k: v for k, v in refused.items() if v != bad}
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((cnt == -77).all()), "a refused call wrote"
    # and what is not refused: far_z == max_depth, band 0, near_z 0, one class, a map that has never been updated
    ok = {"far == max_depth": rc(good_prm(pop, far_z=20.0)), "one class": rc(good_prm(pop, classes=16)), "as is": rc()}
    assert all(v == 0 for v in ok.values()), ok
    torch.cuda.synchronize()
    assert not bool((out == GUARD).any())


def test_every_refusal_of_the_masked_audit(cube_sides):
    import torch
    pop, sogm = _mods()
    lib, abi = pop.lib(), pop._abi
    test, truth = cube_sides
    out = torch.full((3 * 2 * 8,), -77, dtype=torch.int32, device="cuda")
    mask = dev_mask(np.zeros((3, 16, 16, 1), np.uint64))

    def prm(**kw):
        p = abi.SogmMapAuditParams()
        assert lib.sogm_map_audit_default_params(2, 2, C.byref(p)) == 0
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    getattr(p, k)[i] = x
            else:
                setattr(p, k, v)
        return p

    def rc(p=None, a=test.m.ctx, b=truth.m.ctx, k=mask.data_ptr(), o=out.data_ptr(), null_prm=False):
        p = prm() if p is None else p
        return lib.sogm_map_audit_masked(a, b, None if null_prm else C.byref(p), k, o, None, sogm._stream())

    other, never = VSide((16, 16, 14), 2, 3, F32).put(), VSide((16, 16, 16), 2, 3, F32)
    try:
        refused = {"null test": rc(a=None), "null truth": rc(b=None), "null prm": rc(null_prm=True), "null out": rc(o=None),
                   "null mask": rc(k=None), "frustum flag": rc(prm(flags=abi.SOGM_MAPAUDIT_FRUSTUM, far_z=3.0, tan_h=1.0, tan_v=1.0)),
                   "tolerance 4": rc(prm(tolerance=4)), "empty box": rc(prm(box_lo=[2, 0, 0], box_hi=[2, 16, 16])),
                   "slice_map T_truth": rc(prm(slice_map=[2, 0])), "other H": rc(b=other.m.ctx)}
        assert all(v == abi.SOGM_ERR_INVALID_ARG for v in refused.values()), refused
        assert lib.sogm_last_error().startswith(b"sogm_map_audit_masked: ")
        assert rc(b=never.m.ctx) == abi.SOGM_ERR_STATE
        torch.cuda.synchronize()
        assert bool((out == -77).all()), "a refused call wrote rows"
        assert rc(prm(near_z=np.nan, tan_h=-1.0)) == 0                    # the frustum numbers are not read
        torch.cuda.synchronize()
        assert not bool((out.view(3, 2, 8)[:, :, :6] != 0).any())          # an empty mask: an empty region
    finally:
        other.close()
        never.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def test_render_view_mask_audit_chain(pop):
    """one cylinder 0.65 m ahead of two cameras near the centre of a 16^3 map: render_depth -> view_mask -> audit_against(mask=)
    equals the reading made from the downloaded image and grids; the cylinder has an unseen interior (HIDDEN > 0) and the
    visible region holds fewer truth cells than the frustum"""
    _, sogm = _mods()
    depth = importlib.import_module("pred-occ-planner_amd.depth")
    dims, A, T = (16, 16, 16), 2, 2
    test, truth = VSide(dims, T, A, F32), VSide(dims, T, A, F32 | TILED)
    try:
        centre = np.array([[2.0, 1.0, 1.2], [2.0, 1.0, 1.2]], np.float32)
        poses = [pop.scene.camera_pose(2.013, 1.027, 1.231, 0.0), pop.scene.camera_pose(1.9, 0.9, 1.2, 0.2)]
        pos, rot = np.stack([c for c, _ in poses]), np.stack([R.reshape(9) for _, R in poses])
        rec = np.array([fx.cylinder(2.65, 1.05, 0.5, z=1.2, h=1.5)])
        th, zz = np.meshgrid(np.linspace(0, 2 * np.pi, 40, endpoint=False), np.arange(0.5, 1.95, 0.1))
        cloud = np.stack([rec[0, 1] + 0.25 * np.cos(th), rec[0, 2] + 0.25 * np.sin(th), zz], axis=2).reshape(-1, 3).astype(np.float32)
        world = sogm.World(cloud, fx.to_struct(pop._abi, rec), n_cyl=1)
        stamps = np.full(A, 3.0)
        truth.centres, truth.stamps = centre, stamps
        truth.m.updateWorld(world, sogm._dev(centre, np.float32), sogm._dev(stamps, np.float64))
        truth.grids = [truth.m.download(a) for a in range(A)]
        rng = np.random.default_rng(9)
        test.put(values=(rng.random((A, test.V, T)) < 0.1).astype(np.float32), centres=centre, stamps=stamps)
        cam = depth.make_depth_camera(ROWS, COLS, 1.1, 1000.0, 0.0, False, fx=16.0, fy=16.0, cx=15.5, cy=11.5)
        img, _, _, unsupported = depth.render_depth(world, cam, pos, rot, want_cloud=False)
        off = pos - centre.astype(np.float64)
        band = 0.15
        mask, counts = test.m.view_mask(img, cam, rot, band=band, cam_offset=off)
        got = test.m.audit_against(truth.m, tolerance=1, mask=mask)
        # the reading, end to end, from what the device holds
        image = img.cpu().numpy().view(np.uint16)
        assert unsupported.cpu().numpy().tolist() == [0, 0] and (image > 0).any() and (image == 0).any()
        prm = dict(fx=16.0, fy=16.0, cx=15.5, cy=11.5, depth_scale=1000.0, near_z=0.0, far_z=1.1, tan_h=0.5 * COLS / 16.0,
                   tan_v=0.5 * ROWS / 16.0, band=band)
        cls, words, want_n = vref.view_mask(dims, np.float32(0.15), image, rot, prm, VISIBLE, off)
        assert np.array_equal(mask.cpu().numpy().view(np.uint64), words) and np.array_equal(counts.cpu().numpy(), want_n)
        R = (cls == vref.FREE) | (cls == vref.SURFACE)
        thr = test.m.spec.risk_threshold
        want = np.stack([vref.audit_with_region(test.grids[a], truth.grids[a], R[a], dims, thr, thr, 1) for a in range(A)])
        rows = ROW(got)
        print("chain: counts", want_n[:, :6].tolist(), "rows agent 0", rows[0, :, :6].tolist())
        assert np.array_equal(rows, want) and (rows[:, :, 7] == 0).all()
        assert (want_n[:, vref.HIDDEN] > 0).all() and (want_n[:, vref.SURFACE] > 0).all()
        frustum = np.stack([vref.audit_with_region(test.grids[a], truth.grids[a], cls[a] != vref.OUTSIDE, dims, thr, thr, 1)
                            for a in range(A)])
        assert (want[:, 0, 2] < frustum[:, 0, 2]).all() and (want[:, 0, 2] > 0).all()
    finally:
        test.close()
        truth.close()


def test_facade_view_mask_on_gpu(tmp_path):
    out = subprocess.run([build_facade_program(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "view mask facade ok" in out.stdout
