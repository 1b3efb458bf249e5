"""DSPMap::update (row a6) branch by branch against the INDEPENDENT reading (tests/golden/make_dsp_cases_fixture.py ->
dsp_cases_independent.json): hand-built particle stores injected through the state hook (sogm_dsp_upload_state /
orc_dsp_set_state), one named case per branch of prediction + placement, observation binning, mapUpdate, new-born and occupancy +
resample, on two tiny grids.  The C++ oracle on the CPU; sogm_update_dsp directly on the GPU — all cases of one grid as the
agents of one handle — against the reading AND bit for bit against the oracle on the same inputs.

Exact: the return value, every slot's flag, velocity and position bits of every live particle, the cursors, the observation
tables (count, x / y / z / length, max_length), the counters voxel_full / pyramid_full / moved_out, the three error counters.
To the project's tolerances (the reading's normal-PDF table and plane normals come from the interpreter's exp / sin, not glibc's
expf / sinf): EVERY live particle's weight and every C_k (rtol 1e-4), every entry of objnum per voxel (rtol 1e-4, atol 1e-6).
The generator asserts that no tolerance decides anything (its docstring); a failure names the case and the first differing voxel
and slot.

Capacities, read from k_dsp_place / k_dsp_pyramids / k_dsp_commit_slots: round r of the DSP_ROUNDS = 6 place / pyramid rounds
finds the vanish of chain depth r + 1 and the last round must find nothing, so a cascade of 5 is the longest that settles with
counters[10] == 0 (cascade_at_the_limit: exact) and 6 raises it (cascade_one_over_the_limit: the call is OK, the store is not
compared).  The candidate pool holds cand_cap = 2 V movers + in-FOV stays: exactly 2 V is exact with counters[11] == 0, 2 V + 1
gives counters[11] == 1 (k_dsp_predict drops the candidate before any write; k_dsp_commit_movers clamps its count)."""
import base64
import hashlib
import importlib
import json
import os
import zlib

import numpy as np
import pytest

from helpers import DSP_CASE_GRIDS, DSP_CASE_LABELS as ALL_LABELS, dsp_case_inputs, dsp_case_sha256, dsp_case_tables

HERE = os.path.dirname(os.path.abspath(__file__))
S = 14
CAPACITY = {"cascade_one_over_the_limit": 10, "candidate_pool_2V_plus_1": 11}      # the error counter each over-limit case raises
OBSERVED = {}      # the largest differences seen, printed at the end of each test (DESIGN.md section 4 quotes them)

with open(os.path.join(HERE, "golden", "dsp_cases_independent.json")) as _f:
    FX = json.load(_f)
FX_CASES = {c["name"]: c for c in FX["cases"]}
_INPUTS = None

UNCLAIMED = set()      # every label of DSP_CASE_LABELS is claimed by a case


def _inputs():
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = dsp_case_inputs()
    return _INPUTS


def _case(name):
    return next(c for g in _inputs().values() for c in g if c.name == name)


def _unpack(s, dtype, shape):
    a = np.frombuffer(zlib.decompress(base64.b85decode(s)), dtype)
    known = -int(np.prod(shape))      # one entry of shape may be -1 (numpy refuses to infer it for an empty array)
    return a.reshape(tuple(a.size // known if n == -1 else n for n in shape))


def _dense(pair, dtype, shape):
    """an almost empty array from [the gaps between the flat indices of its non-zero entries (int32), those entries]"""
    out = np.zeros(int(np.prod(shape)), dtype)
    out[np.cumsum(_unpack(pair[0], np.int32, (-1,)))] = _unpack(pair[1], dtype, (-1,))
    return out.reshape(shape)


def _note(key, value):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(value))


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def _close(what, got, want, rtol, atol, where, key):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    big = want != 0
    if big.any():
        _note(key, rel[big & (np.abs(want) > 1e-6)].max() if (big & (np.abs(want) > 1e-6)).any() else 0.0)
    bad = ~(err <= atol + rtol * np.abs(want))
    if bad.any():
        at = _first(bad)
        raise AssertionError("%s: %s differs first at %r: got %.9g, want %.9g (rtol %g, atol %g)" % (where, what, at, got[at], want[at], rtol, atol))


def _bits_equal(what, got, want, where):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (where, what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = _first(bad)
        raise AssertionError("%s: %s differs first at (voxel, slot, ...) = %r: got %r, want %r" % (where, what, at, got[at], want[at]))


def _check(name, k, rec, grid, ok, store, objnum, counters, nobs, pc, ml, exact_weights=None):
    """one update of one case against the reading; exact_weights: the oracle's (store, objnum, pc) for the kernel's bit-for-bit check"""
    NX, NY, NZ, T = DSP_CASE_GRIDS[grid]
    V = NX * NY * NZ
    where = "%s update %d" % (name, k)
    assert int(ok) == rec["ok"], (where, "return value", int(ok), rec["ok"])
    want_flags = _dense(rec["flags"], np.float32, (V, S))
    _bits_equal("slot flags", store[:, :, 0], want_flags, where)
    occ = store[:, :, 0] > np.float32(0.1)
    assert int(occ.sum()) == rec["n_particles"], where
    want_live = np.zeros((V, S, 7), np.float32)      # velocity, position and weight of the live slots, in (voxel, slot) order
    want_live[want_flags > np.float32(0.1)] = _unpack(rec["live"], np.float32, (7, -1)).T
    _bits_equal("velocity / position", np.where(occ[:, :, None], store[:, :, 1:7], 0), want_live[:, :, :6], where)
    assert [int(c) for c in counters[4:7]] == rec["cursors"], (where, "cursors", list(counters[4:7]), rec["cursors"])
    assert [int(c) for c in counters[0:3]] == rec["counters"], (where, "voxel_full / pyramid_full / moved_out", list(counters[0:3]), rec["counters"])
    want_nobs = _dense(rec["nobs"], np.int32, (len(nobs),))
    assert np.array_equal(nobs, want_nobs), (where, "nobs differs first at pyramid", _first(nobs != want_nobs))
    pyr = np.flatnonzero(want_nobs)      # max_length is set exactly in the pyramids that hold an observation (the generator asserts it)
    want_ml = np.full(len(ml), -1.0, np.float32)
    want_ml[pyr] = _unpack(rec["maxlen"], np.float32, (-1,))
    _bits_equal("max_length", ml, want_ml, where)
    gather = lambda t: np.concatenate([t[i, :want_nobs[i]] for i in pyr]) if len(pyr) else np.zeros((0, 5), np.float32)
    rows, want_rows = gather(pc), _unpack(rec["obs"], np.float32, (5, -1)).T
    _bits_equal("observation x / y / z / length", rows[:, [0, 1, 2, 4]], want_rows[:, [0, 1, 2, 4]], where)
    # "exact": no listed particle since the store was injected, so no normal-PDF entry has entered any weight or C_k — plain IEEE
    # arithmetic on the inputs, held with no tolerance at all (the generator then asks no margin of the decisions they take)
    rtol, atol = (0.0, 0.0) if rec["exact"] else (1e-4, 1e-6)
    _close("C_k (observation row)", rows[:, 3], want_rows[:, 3], rtol, 0.0, where, "C_k rel")
    _close("weight (voxel, slot)", np.where(occ, store[:, :, 7], 0), want_live[:, :, 6], rtol, 0.0, where, "weight rel")
    _close("objnum (voxel, entry)", objnum, _dense(rec["obj"], np.float32, (V, 4 + T)), rtol, atol, where, "objnum rel")
    if exact_weights is not None:
        o_store, o_objnum, o_pc = exact_weights
        _bits_equal("slot flags against the oracle", store[:, :, 0], o_store[:, :, 0], where)
        _bits_equal("velocity / position against the oracle", np.where(occ[:, :, None], store[:, :, 1:7], 0),
                    np.where(occ[:, :, None], o_store[:, :, 1:7], 0), where)
        _bits_equal("weight against the oracle", np.where(occ, store[:, :, 7], 0), np.where(occ, o_store[:, :, 7], 0), where)
        _bits_equal("objnum against the oracle", objnum, o_objnum, where)
        o_rows = gather(o_pc)
        _bits_equal("C_k against the oracle", rows[:, 3], o_rows[:, 3], where)


def _params(pop, grid):
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    spec = pop.config.make_spec(DSP_CASE_GRIDS[grid])
    spec.map_kind = pop._abi.SOGM_MAP_RISKBASE
    P = dsp.make_dsp_params(spec.T)
    NP = (P.half_fov_h * 2 // P.angle_resolution) * (P.half_fov_v * 2 // P.angle_resolution)
    return spec, P, NP


def _oracle_run(pop, orc, case):
    """[(ok, store, objnum, counters, nobs, pc, maxlen)] per update, from the C++ oracle"""
    spec, P, NP = _params(pop, case.grid)
    o = orc.DspOracle(spec, P, dsp_case_tables())
    assert o.set_state(case.store, case.last_pos, case.last_stamp, case.cursors) == 0
    out = []
    for u in case.updates:
        ok = o.update(u["points"], u["labels"], u["pos"], u["quat"], u["stamp"])
        out.append((ok,) + o.state() + o.observations(NP))
        o.publish(0.7, 0)      # the consumer clears the future status (getOccupancyMapWithFutureStatus, dsp_dynamic.h:454-476)
    o.close()
    return out


def test_fixture_covers_every_branch_and_its_inputs_are_the_builders():
    claimed = {b for c in FX["cases"] for b in c["branches"]}
    assert set(FX["unclaimed"]) == UNCLAIMED and all(len(r) > 20 for r in FX["unclaimed"].values()), FX["unclaimed"]
    assert claimed == set(ALL_LABELS) - UNCLAIMED, (sorted(set(ALL_LABELS) - UNCLAIMED - claimed), sorted(claimed - set(ALL_LABELS)))
    assert FX["grids"] == {k: list(v) for k, v in DSP_CASE_GRIDS.items()}
    names = [c.name for g in _inputs().values() for c in g]
    assert names == [c["name"] for c in FX["cases"]]
    for g in _inputs().values():
        for c in g:
            assert dsp_case_sha256(c) == FX_CASES[c.name]["in_sha256"], c.name
            assert 1 <= len(c.updates) <= 3 and c.compare == FX_CASES[c.name]["compare"]
    # the generator's conditions: no tolerance decides anything
    for key, bound in (("removal", 1e-3), ("resample", 1e-3), ("split_truncation", 1e-3), ("occlusion", 1e-3), ("dot", 1e-5), ("trunc", 1e-4)):
        # (a key is absent when every such decision was taken on "exact" weights, which _check holds with no tolerance)
        assert FX["margins"].get(key, bound) >= bound, (key, FX["margins"][key])
    tables = dsp_case_tables()
    assert hashlib.sha256(b"".join(t.tobytes() for t in tables)).hexdigest()[:16] == FX.get("tables_sha256", "")[:16]


@pytest.mark.parametrize("name", [c["name"] for c in FX["cases"]])
def test_oracle_case(pop, orc, name):
    case, fx = _case(name), FX_CASES[name]
    for k, (res, rec) in enumerate(zip(_oracle_run(pop, orc, case), fx["updates"])):
        if not rec["ok"]:      # a rejected update: 0, and the store stays byte-identical (entry 8 is the oracle's own update time)
            assert res[0] == 0 and np.array_equal(res[1][:, :, :8], case.store[:, :, :8]), name
        _check(name, k, rec, case.grid, *res)
    print("observed maxima:", OBSERVED)


def _bad_stores(case):
    """(what, store, cursors) that the state hook must refuse"""
    v = int(np.argwhere(case.store[:, :, 0] > 0)[0][0])
    out = []
    for what, (slot, entry, value) in (("flag 7", (0, 0, 7.0)), ("flag 15", (0, 0, 15.0)), ("flag 0.5", (0, 0, 0.5)), ("flag NaN", (0, 0, np.nan)),
                                       ("flag -1", (13, 0, -1.0)), ("vz != 0", (0, 3, 0.25)), ("vz NaN", (0, 3, np.nan))):
        st = case.store.copy()
        if st[v, slot, 0] == 0 and entry == 3:
            st[v, slot, 0] = 1.0
        st[v, slot, entry] = value
        out.append((what, st, case.cursors))
    out += [("p cursor", case.store, (4096, 0, 0)), ("v cursor", case.store, (0, -1, 0)), ("rand cursor", case.store, (0, 0, 512))]
    return out


def _roundtrip_store(case):
    """a between-updates store with every legal feature: flags 0 / 0.6 / 1, an ignored entry 8, payload on an empty slot, vz on an empty slot"""
    st = case.store.copy()
    v = int(np.argwhere(st[:, :, 0] > 0)[0][0])
    st[v, 13] = (0.6, 0.25, -0.5, 0.0, 0.1, 0.2, 0.3, 0.0625, 99.0)
    st[v, 12] = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)
    return st


def test_oracle_state_hook_round_trip_and_refusals(pop, orc):
    case = _case("resampling_counts")
    spec, P, NP = _params(pop, case.grid)
    o = orc.DspOracle(spec, P, dsp_case_tables())
    st = _roundtrip_store(case)
    assert o.set_state(st, (0.5, -0.25, 0.125), 12.5, (7, 8, 9)) == 0
    got, objnum, cnt = o.state()
    assert np.array_equal(got[:, :, :8], st[:, :, :8]) and not got[:, :, 8].any() and not objnum.any()
    assert list(cnt[:7]) == [0, 0, 0, 0, 7, 8, 9]
    for what, bad, cur in _bad_stores(case):
        assert o.set_state(bad, (0.0, 0.0, 0.0), 1.0, cur) == -1, what
        got2, _, cnt2 = o.state()
        assert np.array_equal(got2, got) and list(cnt2[:7]) == list(cnt[:7]), what      # refused: nothing changed
    # the pose took effect: the same stamp and position give dt = 0 and no odometry delta, 10.1 m away is a jump
    assert o.update(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), (10.7, -0.25, 0.125), (1, 0, 0, 0), 12.5) == 0
    assert o.update(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), (0.5, -0.25, 0.125), (1, 0, 0, 0), 12.5) == 1
    o.close()


@pytest.mark.gpu
def test_kernel_state_hook_round_trip_and_refusals(pop):
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    case = _case("resampling_counts")
    spec, P, NP = _params(pop, case.grid)
    m = sogm.SogmMap(spec, 3)
    g = dsp.DspMap(m, P, dsp_case_tables(), max_points=64)
    st = _roundtrip_store(case)
    before = [g.download_state(a) for a in range(3)]
    assert g.upload_state(1, st, (0.5, -0.25, 0.125), 12.5, (7, 8, 9)) == pop._abi.SOGM_OK
    got, objnum, cnt = g.download_state(1)
    want = st.copy()
    want[:, :, 8] = 0
    want[:, :, 3] = 0      # vz is not stored: an empty slot's comes back as 0 like everyone's
    assert np.array_equal(got, want) and not objnum.any()
    assert list(cnt[:3]) == [0, 0, 0] and list(cnt[4:7]) == [7, 8, 9] and list(cnt[10:13]) == [0, 0, 0]
    for what, bad, cur in _bad_stores(case):
        assert g.upload_state(1, bad, (0.0, 0.0, 0.0), 1.0, cur) == pop._abi.SOGM_ERR_INVALID_ARG, what
        got2, _, cnt2 = g.download_state(1)
        assert np.array_equal(got2, got) and np.array_equal(cnt2, cnt), what
    assert g.upload_state(3, st, (0.0, 0.0, 0.0), 1.0, (0, 0, 0)) == pop._abi.SOGM_ERR_INVALID_ARG
    assert g.upload_state(-1, st, (0.0, 0.0, 0.0), 1.0, (0, 0, 0)) == pop._abi.SOGM_ERR_INVALID_ARG
    for a in (0, 2):      # the neighbours were never touched
        s2, o2, c2 = g.download_state(a)
        assert np.array_equal(s2, before[a][0]) and np.array_equal(o2, before[a][1]) and np.array_equal(c2, before[a][2])
    # the pose took effect (agent 1): a 10.2 m jump is refused, the injected pose itself is accepted; the others see a first call
    dev = lambda a, t: sogm._dev(np.ascontiguousarray(a, t), t)
    args = lambda pos: (dev(np.zeros((1, 3)), np.float32), dev(np.zeros((1, 4)), np.float32), dev(np.zeros((3, 2)), np.int32),
                        dev([pos] * 3, np.float32), dev([[1, 0, 0, 0]] * 3, np.float32), dev([12.5] * 3, np.float64))
    assert g.update(*args((10.7, -0.25, 0.125))).cpu().numpy().tolist() == [1, 0, 1]
    assert g.update(*args((0.5, -0.25, 0.125))).cpu().numpy().tolist() == [0, 1, 0]      # (10.2 m from the others' first pose)
    assert g.upload_state(0, st, (0.5, -0.25, 0.125), 12.5, (7, 8, 9)) == pop._abi.SOGM_OK
    assert g.update(*args((0.5, -0.25, 0.125))).cpu().numpy().tolist() == [1, 1, 0]
    g.close()
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", sorted(DSP_CASE_GRIDS))
def test_kernel_cases(pop, orc, grid):
    """all cases of one grid as the agents of one handle, update round by update round (an agent whose case has fewer updates is
    given a quaternion the update refuses, which leaves its state alone)"""
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    cases = _inputs()[grid]
    A = len(cases)
    spec, P, NP = _params(pop, grid)
    oracle = {c.name: _oracle_run(pop, orc, c) for c in cases}
    m = sogm.SogmMap(spec, A)
    g = dsp.DspMap(m, P, dsp_case_tables(), max_points=2560)
    for a, c in enumerate(cases):
        assert g.upload_state(a, c.store, c.last_pos, c.last_stamp, c.cursors) == pop._abi.SOGM_OK, c.name
    dev = lambda x, t: sogm._dev(np.ascontiguousarray(x, t), t)
    for k in range(max(len(c.updates) for c in cases)):
        pts, lab, rng, pos, quat, stamp = [np.zeros((1, 3), np.float32)], [np.zeros((1, 4), np.float32)], [], [], [], []
        at = 1
        for c in cases:
            u = c.updates[k] if k < len(c.updates) else {"points": np.zeros((0, 3), np.float32), "labels": np.zeros((0, 4), np.float32),
                                                         "pos": (0, 0, 0), "quat": (2.0, 0, 0, 0), "stamp": 0.0}
            pts.append(u["points"])
            lab.append(u["labels"])
            rng.append((at, at + len(u["points"])))
            at += len(u["points"])
            pos.append(u["pos"])
            quat.append(u["quat"])
            stamp.append(u["stamp"])
        ok = g.update(dev(np.concatenate(pts), np.float32), dev(np.concatenate(lab), np.float32), dev(rng, np.int32), dev(pos, np.float32),
                      dev(quat, np.float32), dev(stamp, np.float64)).cpu().numpy()
        for a, c in enumerate(cases):
            if k >= len(c.updates):
                assert ok[a] == 0
                continue
            store, objnum, cnt = g.download_state(a)
            err = [int(x) for x in cnt[10:13]]
            if not c.compare:      # over a capacity: exactly its counter, the call returned OK, the store is not compared
                i = CAPACITY[c.name]
                assert err[i - 10] != 0 and (i == 10 or err[i - 10] == 1) and sum(1 for x in err if x) == 1, (c.name, err)
                continue
            assert err == [0, 0, 0], (c.name, "error counters", err)
            nobs, pc, ml = g.download_observations(a)
            o = oracle[c.name][k]
            _check(c.name, k, FX_CASES[c.name]["updates"][k], grid, int(ok[a]), store, objnum, cnt, nobs, pc, ml, exact_weights=(o[1], o[2], o[5]))
            assert int(ok[a]) == o[0]
        g.publish()
    g.close()
    m.close()
    print("observed maxima:", OBSERVED)
