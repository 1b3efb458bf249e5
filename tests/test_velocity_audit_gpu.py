"""GPU: the velocity audit (include/sogm_abi.h "velocity audit") — the source index sogm_update_dsp leaves beside the new-born
list, and sogm_dsp_velocity_audit against the numpy reading (tests/velocity_audit_reference.py).  All 29 sequences of
helpers.velocity_fixture_inputs() are the agents of one handle on the parity grid (their LAST frames fall on the same update, so
one audit scores them all), with the seeded truth arrays of tests/velocity_audit_fixtures.py; a second handle is given labels
on that last update.  tests/test_velocity_audit_host.py asserts, on the CPU, that these inputs fill every class and bin."""
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import ring_fixtures as fx  # noqa: E402
import velocity_audit_fixtures as vfx  # noqa: E402
import velocity_audit_reference as vref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRM = dict(speed_tolerance=vfx.TOLERANCE, n_codes=vfx.N_CODES)


def _mods():
    return (importlib.import_module("pred-occ-planner_amd"), importlib.import_module("pred-occ-planner_amd.sogm"),
            importlib.import_module("pred-occ-planner_amd.dsp"))


def _update(sogm, g, frames, labels=None):
    """one sogm_update_dsp over the agents' frames; returns (ok, the device range)"""
    pts = [f["points"] for f in frames]
    ends = np.cumsum([len(p) for p in pts])
    rng = sogm._dev(np.stack([np.concatenate([[0], ends[:-1]]), ends], axis=1).astype(np.int32), np.int32)
    allp = np.concatenate(pts) if ends[-1] else np.zeros((1, 3), np.float32)
    ok = g.update(sogm._dev(allp, np.float32), None if labels is None else sogm._dev(labels, np.float32), rng,
                  sogm._dev(np.float32([f["pos"] for f in frames]), np.float32), sogm._dev(np.float32([f["quat"] for f in frames]), np.float32),
                  sogm._dev(np.asarray([f["stamp"] for f in frames], np.float64), np.float64))
    return ok.cpu().numpy(), rng


class Rig:
    """both handles after the sequences' last frames, and everything the tests compare, computed once"""

    def __init__(self):
        pop, sogm, dsp = _mods()
        self.sogm = sogm
        seqs = helpers.velocity_fixture_inputs()
        self.seqs, A = seqs, len(seqs)
        spec = pop.config.make_spec("parity", map_kind=2)
        params, tabs = dsp.make_dsp_params(spec.T), dsp.make_tables(11, n_gauss=1 << 16, n_rand=1 << 12)
        self.m, self.m2 = sogm.SogmMap(spec, A), sogm.SogmMap(spec, A)
        self.g, self.g2 = dsp.DspMap(self.m, params, tabs), dsp.DspMap(self.m2, params, tabs)
        truth = [vfx.truth_arrays(a, len(s["frames"][-1]["points"])) for a, s in enumerate(seqs)]
        self.labels = [t[0] for t in truth]
        self.codes = [t[1] for t in truth]
        self.clean = [np.where(np.isnan(l).any(axis=1, keepdims=True), np.float32(0), l) for l in self.labels]   # what a map is fed
        steps = max(len(s["frames"]) for s in seqs)
        for k in range(steps):
            frames = []
            for s in seqs:
                i = k - (steps - len(s["frames"]))     # a sequence starts late: empty clouds at its first pose and stamp before
                frames.append(s["frames"][i] if i >= 0 else dict(s["frames"][0], points=np.zeros((0, 3), np.float32)))
            last = k == steps - 1
            ok, self.range = _update(sogm, self.g, frames)
            ok2, _ = _update(sogm, self.g2, frames, np.concatenate(self.clean) if last else None)
            assert ok.tolist() == ok2.tolist() == [1] * A
        self.n_in = [len(l) for l in self.labels]
        self.labels_d = sogm._dev(np.concatenate(self.labels), np.float32)
        self.clean_d = sogm._dev(np.concatenate(self.clean), np.float32)
        self.codes_d = sogm._dev(np.concatenate(self.codes), np.int32)
        self.born = [self.g.download_born(a)[0] for a in range(A)]
        self.src = [self.g.download_born_source(a) for a in range(A)]
        self.born2 = [self.g2.download_born(a)[0] for a in range(A)]
        self.src2 = [self.g2.download_born_source(a) for a in range(A)]
        self.want = [vref.audit_agent(self.born[a], self.src[a], self.n_in[a], self.labels[a], self.codes[a], PRM) for a in range(A)]

    def audit(self, g=None, labels=None, codes="own", **kw):
        rows, table = (g or self.g).audit_velocity(self.labels_d if labels is None else labels,
                                                   self.codes_d if isinstance(codes, str) else codes, self.range, **kw)
        return rows.cpu().numpy(), None if table is None else table.cpu().numpy()

    def close(self):
        for x in (self.g, self.g2, self.m, self.m2):
            x.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


# ---- 1. the source index -----------------------------------------------------------------------------------------------------
def test_source_index_of_the_estimators_list(rig):
    with open(os.path.join(ROOT, "tests", "golden", "velocity_independent.json")) as f:
        golden = json.load(f)["sequences"]
    dropped_total = 0
    for a, s in enumerate(rig.seqs):
        src, born, n_in = rig.src[a], rig.born[a], rig.n_in[a]
        where = s["branch"]
        assert len(src) == len(born) and len(np.unique(src)) == len(src), where                      # injective
        assert len(src) == 0 or (src.min() >= 0 and src.max() < n_in), where
        # row k is input point src[k], bit for bit: the labels-given list is the rotated, translated cloud in input order
        assert rig.born2[a].shape == (n_in, 7) and np.array_equal(rig.src2[a], np.arange(n_in)), where
        assert np.array_equal(born[:, :3].view(np.uint32), rig.born2[a][src, :3].view(np.uint32)), where
        assert np.array_equal(rig.born2[a][:, 3:].view(np.uint32), rig.clean[a].view(np.uint32)), where
        # the points no row names are the members of rejected clusters: as many as the independent reading drops
        e = golden[a]["frames"][-1]
        assert e["n"] == n_in and len(born) == e["n_born"], (where, n_in, len(born), e["n"], e["n_born"])
        dropped_total += n_in - len(src)
    by = {s["branch"]: a for a, s in enumerate(rig.seqs)}
    assert rig.n_in[by["size_4_dropped_5_kept"]] - len(rig.src[by["size_4_dropped_5_kept"]]) == 4 and dropped_total >= 4
    for name in ("cloud_1025", "cloud_2600", "rotated_moving_sensor"):        # the second and third trip, the rotated sensor
        a = by[name]
        assert not np.array_equal(rig.src[a], np.arange(len(rig.src[a]))) and len(rig.src[a]) == rig.n_in[a], name
    assert rig.src[by["cloud_2600"]].max() == 2599


# ---- 2. rows and per-code tables ---------------------------------------------------------------------------------------------
def test_rows_and_tables_equal_the_reading(rig):
    rows, table = rig.audit(n_codes=vfx.N_CODES, speed_tolerance=vfx.TOLERANCE, per_code=True)
    assert rows.shape == (len(rig.seqs), 32) and table.shape == (len(rig.seqs), vfx.N_CODES + 2, 6)
    total = np.zeros(32, np.int64)
    for a, s in enumerate(rig.seqs):
        wr, wt = rig.want[a]
        assert rows[a].tolist() == wr.tolist(), (s["branch"], rows[a].tolist(), wr.tolist())
        assert np.array_equal(table[a], wt), (s["branch"], table[a].tolist(), wt.tolist())
        total += rows[a]
    print("summed row:", total.tolist())
    assert (total[4:12] > 0).all() and (total[12:18] > 0).all() and (total[24:29] > 0).all() and total[3] > 0
    # without the table the rows are the same; so they are with another n_codes
    rows2, none = rig.audit(codes=None, n_codes=0, speed_tolerance=vfx.TOLERANCE)
    assert none is None and np.array_equal(rows2, rows)
    # another tolerance and another n_codes against the reading
    prm = dict(speed_tolerance=0.5, n_codes=3)
    rows3, table3 = rig.audit(per_code=True, **prm)
    for a in (0, 13, 15, 26):
        wr, wt = vref.audit_agent(rig.born[a], rig.src[a], rig.n_in[a], rig.labels[a], rig.codes[a], prm)
        assert rows3[a].tolist() == wr.tolist() and np.array_equal(table3[a], wt), rig.seqs[a]["branch"]


# ---- 3. a labels-given update against its own labels -------------------------------------------------------------------------
def test_labels_given_update_scores_itself_perfectly(rig):
    rows, table = rig.audit(g=rig.g2, labels=rig.clean_d, n_codes=vfx.N_CODES, speed_tolerance=0.0, per_code=True)
    for a, s in enumerate(rig.seqs):
        r = rows[a]
        moving = int((rig.clean[a][:, 3] > 0.01).sum())
        conf = r[4:12].reshape(2, 4)
        assert r[0] == r[1] == rig.n_in[a] and r[2] == 0 and r[3] == 0, s["branch"]
        assert conf.tolist() == [[rig.n_in[a] - moving, 0, 0, 0], [0, moving, 0, 0]], (s["branch"], conf.tolist())
        assert r[12] == moving and not r[13:24].any() and r[24] == moving and not r[25:29].any(), s["branch"]
        assert r[29] == 0 and r[30] == moving and r[31] == 0
        assert table[a][:, 5].sum() == 0 and table[a][:, 4].sum() == moving and table[a][:, 3].sum() == 0


# ---- 4. accumulation ---------------------------------------------------------------------------------------------------------
def _raw(pop, rig, rows, table, labels, flags):
    prm = pop._abi.SogmVelAuditParams()
    prm.speed_tolerance, prm.n_codes, prm.flags = vfx.TOLERANCE, vfx.N_CODES, flags
    pop._abi.check(pop.lib().sogm_dsp_velocity_audit(rig.g._h, labels.data_ptr(), rig.codes_d.data_ptr(), rig.range.data_ptr(),
                                                     C.byref(prm), rows.data_ptr(), table.data_ptr(), rig.sogm._stream()), "audit")


def test_accumulate_adds_and_a_plain_call_overwrites(rig):
    import torch
    pop = _mods()[0]
    kw = dict(n_codes=vfx.N_CODES, speed_tolerance=vfx.TOLERANCE, per_code=True)
    r1, t1 = rig.audit(**kw)
    r2, t2 = rig.audit(labels=rig.clean_d, **kw)
    assert not np.array_equal(r1, r2)                                       # the NaN rows differ
    rows, table = rig.g.audit_velocity(rig.labels_d, rig.codes_d, rig.range, **kw)
    back = rig.g.audit_velocity(rig.clean_d, rig.codes_d, rig.range, accumulate_into=(rows, table), **kw)
    assert back[0] is rows and back[1] is table
    want = r1 + r2
    want[:, 2] = r1[:, 2] | r2[:, 2]
    assert np.array_equal(rows.cpu().numpy(), want) and np.array_equal(table.cpu().numpy(), t1 + t2)
    # the status is ORed, not added: a stale CLIPPED bit stays beside what the call finds, a stale count is added to
    rows.fill_(0)
    rows[:, 2] = 4
    rig.g.audit_velocity(rig.labels_d, rig.codes_d, rig.range, accumulate_into=(rows, table), **kw)
    assert (rows.cpu().numpy()[:, 2] == (r1[:, 2] | 4)).all()
    # a plain call overwrites whatever the outputs held
    stale_r = torch.full((len(rig.seqs), 32), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    stale_t = torch.full((len(rig.seqs), vfx.N_CODES + 2, 6), -7, dtype=torch.int64, device="cuda")
    _raw(pop, rig, stale_r, stale_t, rig.labels_d, 0)
    assert np.array_equal(stale_r.cpu().numpy(), r1) and np.array_equal(stale_t.cpu().numpy(), t1)


# ---- 5. run-to-run stability -------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(rig):
    kw = dict(n_codes=vfx.N_CODES, speed_tolerance=vfx.TOLERANCE, per_code=True)
    a, b = rig.audit(**kw), rig.audit(**kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 6. the handle is untouched ----------------------------------------------------------------------------------------------
def test_the_audit_writes_nothing_to_the_handle(rig):
    agents = (0, 15, 16)
    before = [(rig.g.download_born(a), rig.g.download_born_source(a), rig.g.download_state(a)) for a in agents]
    rig.audit(n_codes=vfx.N_CODES, speed_tolerance=vfx.TOLERANCE, per_code=True)
    for a, (born, src, state) in zip(agents, before):
        b2, s2, st2 = rig.g.download_born(a), rig.g.download_born_source(a), rig.g.download_state(a)
        assert born[0].tobytes() == b2[0].tobytes() and born[1] == b2[1] and src.tobytes() == s2.tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(state, st2))


# ---- 7. skipped agents -------------------------------------------------------------------------------------------------------
def test_skipped_agents_report_zeros():
    pop, sogm, dsp = _mods()
    spec = pop.config.make_spec("parity", map_kind=2)
    m = sogm.SogmMap(spec, 4)
    g = dsp.DspMap(m, dsp.make_dsp_params(spec.T), dsp.make_tables(11, n_gauss=1 << 16, n_rand=1 << 12), max_points=16)
    try:
        fr = helpers.velocity_fixture_inputs()[0]["frames"][0]              # 24 points: longer than max_points = 16
        n = len(fr["points"])
        labels, codes = vfx.truth_arrays(0, 3 * n)
        lab_d, cod_d = sogm._dev(labels, np.float32), sogm._dev(codes, np.int32)
        rng = sogm._dev(np.int32([[0, n], [n, 2 * n], [2 * n, 2 * n], [2 * n, 2 * n + 9]]), np.int32)
        rows, table = g.audit_velocity(lab_d, cod_d, rng, n_codes=vfx.N_CODES, per_code=True)       # before any update: never ran
        assert (rows.cpu().numpy()[:, 2] == 1).all() and not np.delete(rows.cpu().numpy(), 2, axis=1).any() and not table.cpu().numpy().any()
        # agent 0: accepted and clipped; agent 1: rejected (a quaternion component above 1.001); agent 2: an empty range
        frames = [fr, dict(fr, quat=np.float32([1.5, 0, 0, 0])), dict(fr, points=np.zeros((0, 3), np.float32)), dict(fr, points=fr["points"][:9])]
        ok, rng2 = _update(sogm, g, frames)
        assert ok.tolist() == [1, 0, 1, 1] and np.array_equal(rng2.cpu().numpy(), rng.cpu().numpy())
        rows, table = g.audit_velocity(lab_d, cod_d, rng, n_codes=vfx.N_CODES, per_code=True)
        rows, table = rows.cpu().numpy(), table.cpu().numpy()
        for a in (1, 2):
            assert rows[a, 2] == 1 and not np.delete(rows[a], 2).any() and not table[a].any(), a
        for a, lo, length in ((0, 0, n), (3, 2 * n, 9)):
            born, src = g.download_born(a)[0], g.download_born_source(a)
            wr, wt = vref.audit_agent(born, src, None, labels[lo:], codes[lo:], PRM, range_len=length, max_points=16)
            assert rows[a].tolist() == wr.tolist() and np.array_equal(table[a], wt), a
        assert rows[0, 2] == 4 and rows[0, 0] == 16 and rows[3, 2] == 0 and rows[3, 0] == 9
    finally:
        g.close()
        m.close()


# ---- 8. a short chain --------------------------------------------------------------------------------------------------------
def test_a_short_perception_chain(pop):
    """two agents, a 24 x 32 camera with the ground, two moving cylinders: two frames of render(want_hit) -> labelled filter ->
    sogm_update_dsp(labels = NULL) -> audit with the scene's n_codes.  No quality figure is asserted."""
    import torch
    _, sogm, dsp = _mods()
    depth = importlib.import_module("pred-occ-planner_amd.depth")
    rows_, cols, cap, A = 24, 32, 1024, 2
    poses = [pop.scene.camera_pose(0.013, 0.027, 1.031, 0.0), pop.scene.camera_pose(0.493, -0.417, 1.217, 0.1)]
    pos, rot = np.stack([c for c, _ in poses]), np.stack([R.reshape(9) for _, R in poses])
    yaw = np.array([0.0, 0.1])
    spec = pop.config.make_spec("parity", map_kind=pop._abi.SOGM_MAP_RISKVOXEL)
    m = sogm.SogmMap(spec, A)
    g = dsp.DspMap(m, dsp.make_dsp_params(spec.T), dsp.make_tables(5, n_gauss=1 << 16, n_rand=1 << 12), max_points=cap)
    dcam = depth.make_depth_camera(rows_, cols, 4.0, 1000.0, 0.0, True, fx=19.0, fy=19.0, cx=16.0, cy=12.0)
    try:
        pos_d, rot_d = sogm._dev(pos, np.float64), sogm._dev(rot, np.float64)
        base = torch.arange(A, dtype=torch.int32, device="cuda") * cap
        quat = sogm._dev(np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], axis=1), np.float32)
        acc = None
        for k in range(2):
            t = 10.0 + 0.1 * k
            rec = np.array([fx.cylinder(2.531 + 0.37 * 0.1 * k, 0.287 - 0.21 * 0.1 * k, 0.5, z=0.9, h=1.8, vx=0.37, vy=-0.21),
                            fx.cylinder(2.1, -0.9 + 0.5 * 0.1 * k, 0.3, z=0.9, h=1.8, vx=0.0, vy=0.5)])
            world = sogm.World(np.zeros((0, 3), np.float32), fx.to_struct(pop._abi, rec), n_cyl=2)
            _, cl, raw_rng, _, hit = depth.render_depth_swarm(world, dcam, pos_d, rot_d, None, want_hit=True)
            pts, cnt, lab, code = m.filterPointCloudLabelled(cl, hit, raw_rng, world, None, 0.0, 0.15, cap, want_code=True)
            crange = torch.stack([base, base + cnt], dim=1).contiguous()
            ok = g.update(pts.view(-1, 3), None, crange, sogm._dev(pos.astype(np.float32), np.float32), quat,
                          sogm._dev(np.full(A, t), np.float64))
            assert ok.cpu().numpy().tolist() == [1, 1]
            acc = g.audit_velocity(lab.view(-1, 4), code.view(-1), crange, n_codes=2, per_code=True, accumulate_into=acc)
            n = last_n = cnt.cpu().numpy()
            last_rows = g.audit_velocity(lab.view(-1, 4), None, crange)[0].cpu().numpy()
            assert (last_n > 0).all() and last_rows[:, 0].tolist() == last_n.tolist()
            assert last_rows[:, 4:12].sum(axis=1).tolist() == last_n.tolist() and (last_rows[:, 2] == 0).all()
            labs, codes = lab.cpu().numpy(), code.cpu().numpy()
            for a in range(A):                                             # and the reading, on a real cloud
                wr, wt = vref.audit_agent(g.download_born(a)[0], g.download_born_source(a), int(n[a]), labs[a], codes[a],
                                          dict(speed_tolerance=0.25, n_codes=2))
                assert last_rows[a].tolist() == wr.tolist(), a
        rows, table = acc[0].cpu().numpy(), acc[1].cpu().numpy()
        print("chain, summed row:", rows.sum(axis=0).tolist(), dsp.velocity_scores(rows))
        assert table[:, :, :4].sum() == rows[:, 0].sum() and table[:, 2, :4].sum() > 0       # the ground is seen
    finally:
        g.close()
        m.close()


# ---- the C++ facade ----------------------------------------------------------------------------------------------------------
def test_facade_audit_velocity(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "velaudit_facade_gpu_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "velaudit_facade_gpu_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "velocity audit facade ok" in out.stdout
