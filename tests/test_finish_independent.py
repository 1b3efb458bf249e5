"""How a replan ends — ParticleATC::isSafeAfterOpt against the swarm table, the outcome, the record, its publication —
in BOTH device forms (sogm_finish_batched: the grouped kernels k_safe_after_opt + k_pack_records, and the finishing wave
finish_agent that sogm_replan's dataflow and sogm_flight_run inline), held to tests/golden/finish_independent.json, a second
reading written from the reference's text (tests/golden/make_finish_fixture.py; separability by scipy HiGHS, every pair
separable or overlapping by >= 1e-3).  The tables have 1, 63, 64, 65, 128 and 130 records, so the wave's 64-record chunks,
its walk in record order and the restaging of set A behind an LP all run under a check; the capacity groups reach the
largest LP (140 + 8 rows) and the capacity rule with its counter.  Verdicts, flags and counters are integers and the
reading emits exact doubles: every comparison is exact."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CATS = {"f": "far", "i": "inactive", "o": "own", "l": "lp_safe", "u": "unsafe", "c": "capacity"}
PUB_MODES = ("own+table", "own", "table", "none")


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(HERE, "golden", "finish_independent.json")))


@pytest.fixture(scope="module")
def fx_sao():
    return json.load(open(os.path.join(HERE, "golden", "safe_after_opt_independent.json")))


def swarm_groups(fx):
    return [(gi, g) for gi, g in enumerate(fx["groups"]) if g["kind"] != "publication"]


def _records(pop, recs, n=None):
    """a ctypes table of len(recs) (or n) SogmTrajRecord; None entries stay empty (n_pieces 0: inactive)"""
    out = (pop._abi.SogmTrajRecord * max(n or len(recs), 1))()
    for r, rec in zip(out, recs):
        if rec is None:
            continue
        r.drone_id, r.n_pieces, r.time_start = rec["drone_id"], rec["n_pieces"], rec["time_start"]
        for k, d in enumerate(rec["duration"]):
            r.duration[k] = d
        for k, v in enumerate(rec["cpts"]):
            r.cpts[k] = v
    return out


def _bytes(pop, table, n):
    return np.frombuffer(bytes(table), np.uint8)[:n * pop._abi.TRAJ_RECORD_BYTES].reshape(n, pop._abi.TRAJ_RECORD_BYTES).copy()


def ego_cpts(g, e):
    c = np.zeros(16 * 15)
    src = e["cpts"] if e["cpts"] is not None else g["cpts"]
    c[:len(src)] = src
    return c


def expected_out(pop, g, e):
    """the reading's record as bytes"""
    o = e["out"]
    rec = {"drone_id": o["drone_id"], "n_pieces": o["n_pieces"], "time_start": o["time_start"], "duration": o["duration"],
           "cpts": ego_cpts(g, e)[:o["n_cpts"]].tolist()}
    return _bytes(pop, _records(pop, [rec]), 1)[0]


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_bookkeeping(fx):
    groups = fx["groups"]
    assert {g["kind"] for g in groups} == {"chunk", "capacity", "early_exit", "publication"}
    assert {g["n_swarm"] for g in groups if g["kind"] == "chunk"} == {1, 63, 64, 65, 128, 130}
    swarm = [e for _, g in swarm_groups(fx) for e in g["egos"]]
    n_safe = sum(e["safe"] for e in swarm)
    assert 0.25 <= n_safe / len(swarm) <= 0.75, (n_safe, len(swarm))
    cats = "".join(e["pair_cat"] for g in groups for e in g["egos"])
    assert set(cats) == set(CATS) and all(cats.count(c) > 0 for c in CATS)
    assert {1, 8, 16} <= {e["npoly"] for g in groups if g["kind"] == "chunk" for e in g["egos"]}
    only_unsafe_at = set()
    for g in groups:
        assert len(g["egos"]) <= 16 and len(g["records"]) == g["n_swarm"] <= 130
        counts = dict.fromkeys(fx["outcomes"], 0)
        for e in g["egos"]:
            M = e["npoly"]
            if M > 0:
                assert len(e["pair_cat"]) == len(e["pair_safe"]) == len(e["pair_piece"]) == g["n_swarm"]
                assert e["safe"] == int(all(s == "1" for s in e["pair_safe"]))
                for c, s, p, r in zip(e["pair_cat"], e["pair_safe"], e["pair_piece"], g["records"]):
                    assert (s == "0") == (c in "uc") and (p < 0) == (c in "io")
                    if c == "c":
                        assert 5 * M + 5 * (r["n_pieces"] - p) > fx["capacity_rows"]
                if e["pair_cat"].count("u") == 1 and g["kind"] == "chunk":
                    only_unsafe_at.add(e["pair_cat"].index("u"))
            assert e["solved"] == int(e["ret"] != 0 and M > 0 and e["status"] in (1, 2))
            assert e["ok"] == int(e["solved"] and e["safe"]) == int(e["outcome"] == 0)
            assert e["out"]["n_pieces"] == (M if e["ok"] else 0) and e["out"]["n_cpts"] == 15 * e["out"]["n_pieces"]
            assert e["out"]["duration"] == [fx["tau"]] * e["out"]["n_pieces"]
            if e["due"] is None or e["due"] != 0:
                counts[fx["outcomes"][e["outcome"]]] += 1
        assert counts == g["counts"]
        n_cap = sum(e["pair_cat"].count("c") for e in g["egos"])
        assert g["capacity_all"] == n_cap
        assert g["capacity_sequential"] == (n_cap if g["kind"] == "capacity" else 0)
    assert only_unsafe_at >= {0, 62, 63, 64, 127, 128, 129}
    pub = [e for g in groups if g["kind"] == "publication" for e in g["egos"]]
    assert len({(e["ret"], e["npoly"], e["status"], e["safe"] if e["npoly"] else 2, e["due"]) for e in pub}) >= 2 * 3 * 4 * 2 * 3
    assert len(pub) == 2 * 4 * 4 * 2 * 3 and {e["due"] for e in pub} == {None, 0, 1}


def test_oracle_matches_second_reading(pop, orc, fx):
    cap = fx["capacity_rows"]
    assert cap == 144
    for gi, g in swarm_groups(fx):
        L = g["n_swarm"]
        recs = _records(pop, g["records"])
        ones = [_records(pop, [r]) for r in g["records"]]
        for ei, e in enumerate(g["egos"]):
            c = ego_cpts(g, e)
            assert orc.safe_after_opt(c, e["npoly"], recs, L, e["drone_id"], e["t_now"], cap) == e["safe"], (gi, ei)
            for ri in range(L):  # one record at a time: a wrong verdict cannot hide behind another record
                want = int(e["pair_safe"][ri])
                assert orc.safe_after_opt(c, e["npoly"], ones[ri], 1, e["drone_id"], e["t_now"], cap) == want, (gi, ei, ri)
                if e["pair_cat"][ri] in "flu":  # the verdict is the separability of exactly the points the reading names
                    tail = np.asarray(g["records"][ri]["cpts"]).reshape(-1, 3)[e["pair_piece"][ri] * 5:]
                    assert orc.separable(c.reshape(-1, 3)[:5 * e["npoly"]], tail) == want, (gi, ei, ri)


# ------------------------------------------------------------------------------------------------ GPU
class Rig:
    """a planner for its counters, and sogm_finish_batched on a group's inputs"""

    def __init__(self, pop, fx):
        self.pop, self.fx = pop, fx
        self.sogm = importlib.import_module("pred-occ-planner_amd.sogm")
        self.planner = importlib.import_module("pred-occ-planner_amd.planner")
        self.map = self.sogm.SogmMap(pop.config.make_spec("parity"), 1)
        self.P = self.planner.SogmPlanner(self.map, pop.config.make_astar_params(), pop.config.make_planner_params(True),
                                          pop.config.make_qp_settings())
        self.prev = {k: _bytes(pop, _records(pop, fx[k]), 16) for k in ("prev_own", "prev_table")}

    def close(self):
        self.P.close()
        self.map.close()

    def inputs(self, g, egos=None):
        """device inputs of a group's egos (fields: those of the fixture's egos)"""
        dev = self.sogm._dev
        egos = g["egos"] if egos is None else egos
        i32 = lambda k: dev(np.array([e[k] for e in egos], np.int32), np.int32)
        f64 = lambda k: dev(np.array([e[k] for e in egos], np.float64), np.float64)
        due = None if egos[0]["due"] is None else i32("due")
        return {"n": len(egos), "ret": i32("ret"), "npoly": i32("npoly"), "status": i32("status"),
                "cpts": dev(np.stack([ego_cpts(g, e) for e in egos]), np.float64), "ids": i32("drone_id"),
                "now": f64("t_now"), "t_start": f64("t_start"), "due": due}

    def run(self, inp, table, n_swarm, wave, mode="own+table", tau=None):
        """table: device uint8 [n_swarm, 2064] or None.  Returns the outputs as numpy and the counters' rise."""
        import torch
        n, B = inp["n"], self.pop._abi.TRAJ_RECORD_BYTES
        out = torch.full((n, B), 0xA5, dtype=torch.uint8, device="cuda")
        ok = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        safe = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        own = self.sogm._dev(self.prev["prev_own"][:n], np.uint8) if "own" in mode else None
        tab = self.sogm._dev(self.prev["prev_table"][:n], np.uint8) if "table" in mode else None
        self.P.counters(reset=True)
        self.planner.finish_batched(self.fx["tau"] if tau is None else tau, inp["ret"], inp["npoly"], inp["status"],
                                    inp["cpts"], inp["t_start"], inp["ids"], out, ok, safe, swarm=table, n_swarm=n_swarm,
                                    swarm_ego=inp["ids"], swarm_now=inp["now"], due=inp["due"], pub_own=own, pub_table=tab,
                                    planner=self.P, wave=wave)
        cnt = self.P.counters()
        return {"out": out.cpu().numpy(), "ok": ok.cpu().numpy(), "safe": safe.cpu().numpy(),
                "own": own.cpu().numpy() if own is not None else None, "table": tab.cpu().numpy() if tab is not None else None,
                "counters": cnt}


@pytest.fixture(scope="module")
def rig(pop, fx):
    r = Rig(pop, fx)
    yield r
    r.close()


@pytest.fixture(scope="module")
def runs(pop, fx, rig):
    """every group once per form, both tables given: {(group index, wave): outputs}"""
    res = {}
    for gi, g in enumerate(fx["groups"]):
        inp = rig.inputs(g)
        table = rig.sogm._dev(_bytes(pop, _records(pop, g["records"]), g["n_swarm"]), np.uint8)
        for wave in (False, True):
            res[gi, wave] = rig.run(inp, table, g["n_swarm"], wave)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("wave", [False, True], ids=["grouped", "wave"])
def test_verdicts_match_second_reading(fx, runs, wave):
    for gi, g in enumerate(fx["groups"]):
        got = runs[gi, wave]
        print(gi, g["kind"], g["n_swarm"], "ok", got["ok"].tolist(), "safe", got["safe"].tolist())
        assert got["ok"].tolist() == [e["ok"] for e in g["egos"]], (gi, g["kind"], g["n_swarm"])
        for a, e in enumerate(g["egos"]):
            if e["solved"]:
                assert got["safe"][a] == e["safe"], (gi, g["kind"], g["n_swarm"], a, e["pair_cat"])


@pytest.mark.gpu
@pytest.mark.parametrize("wave", [False, True], ids=["grouped", "wave"])
def test_one_record_at_a_time(pop, fx, rig, wave):
    """the record KEPT AT ITS TABLE PLACE (it stays in its 64-record chunk), every other place inactive"""
    import torch
    for gi, g in swarm_groups(fx):
        L = g["n_swarm"]
        inp = rig.inputs(g)
        full = rig.sogm._dev(_bytes(pop, _records(pop, g["records"]), L), np.uint8)
        table = torch.zeros_like(full)
        for ri in range(L):
            table[ri] = full[ri]
            got = rig.run(inp, table, L, wave)
            table[ri] = 0
            want = [int(e["pair_safe"][ri]) for e in g["egos"]]
            assert got["safe"].tolist() == want and got["ok"].tolist() == want, (gi, g["kind"], L, ri, got["safe"].tolist())
            n_cap = sum(e["pair_cat"][ri] == "c" for e in g["egos"])
            assert got["counters"]["deconflict_capacity"] == n_cap, (gi, ri)


@pytest.mark.gpu
def test_existing_fixture_through_the_wave(pop, fx_sao, rig):
    """safe_after_opt_independent.json's timing boundaries, own_record and foreign_at_index cases reach the wave's
    one-lane-per-record restatement of those rules"""
    import torch
    for gi, g in enumerate(fx_sao["groups"]):
        egos = [{"drone_id": e["drone_id"], "t_now": e["t_now"], "t_start": e["t_now"], "ret": 1, "npoly": e["npoly"],
                 "status": 1, "due": None, "cpts": e["cpts"]} for e in g["egos"]]
        inp = rig.inputs(g, egos)
        L = len(g["records"])
        full = rig.sogm._dev(_bytes(pop, _records(pop, g["records"]), L), np.uint8)
        got = rig.run(inp, full, L, True)
        assert got["safe"].tolist() == got["ok"].tolist() == [e["safe"] for e in g["egos"]], (gi, got["safe"].tolist())
        table = torch.zeros_like(full)
        for ri in range(L):
            table[ri] = full[ri]
            got = rig.run(inp, table, L, True)
            table[ri] = 0
            assert got["safe"].tolist() == [e["pairs"][ri]["safe"] for e in g["egos"]], (gi, ri, got["safe"].tolist())
            one = rig.run(inp, full[ri:ri + 1].contiguous(), 1, True)  # ... and alone at place 0, as the grouped test has it
            assert one["safe"].tolist() == got["safe"].tolist(), (gi, ri)


@pytest.mark.gpu
def test_the_two_forms_agree(fx, runs):
    for gi, g in enumerate(fx["groups"]):
        a, b = runs[gi, False], runs[gi, True]
        for k in ("out", "ok", "own", "table"):
            assert np.array_equal(a[k], b[k]), (gi, g["kind"], k)
        outcome = {k: v for k, v in a["counters"].items() if k != "deconflict_capacity"}
        assert outcome == {k: v for k, v in b["counters"].items() if k != "deconflict_capacity"}, (gi, g["kind"])
        if g["kind"] != "early_exit":  # (there the wave has left the loop, as the reference's has: test_counters)
            assert a["counters"]["deconflict_capacity"] == b["counters"]["deconflict_capacity"], (gi, g["kind"])
        for i, e in enumerate(g["egos"]):
            if e["solved"]:
                assert a["safe"][i] == b["safe"][i], (gi, i)
            else:  # the wave skips the check of an agent that fails anyway: only the outcome is the same
                assert a["ok"][i] == b["ok"][i] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("wave", [False, True], ids=["grouped", "wave"])
def test_counters(fx, runs, wave):
    for gi, g in enumerate(fx["groups"]):
        cnt = runs[gi, wave]["counters"]
        print(gi, g["kind"], cnt)
        assert {k: cnt[k] for k in fx["outcomes"]} == g["counts"], (gi, g["kind"])
        # the wave walks the table as the reference does and has returned at the first unsafe record; the grouped form
        # tests every pair.  The capacity groups are built so that both count every over-capacity pair.
        want = g["capacity_sequential"] if wave else g["capacity_all"]
        assert cnt["deconflict_capacity"] == want, (gi, g["kind"], cnt["deconflict_capacity"], want)
        if g["kind"] in ("chunk", "publication"):
            assert want == 0
        assert cnt["corridor_capacity"] == cnt["pieces_capacity"] == 0


def _check_records(pop, rig, g, got, mode, where):
    new = [expected_out(pop, g, e) for e in g["egos"]]
    for a, e in enumerate(g["egos"]):
        assert np.array_equal(got["out"][a], new[a]), (where, a, "out")
        for key, tag in zip(("own", "table"), e["pub"][mode]):
            if tag is None:
                assert got[key] is None
                continue
            want = new[a] if tag == "new" else rig.prev[tag][a]
            assert np.array_equal(got[key][a], want), (where, a, key, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("wave", [False, True], ids=["grouped", "wave"])
def test_records_and_publication(pop, fx, rig, runs, wave):
    for gi, g in enumerate(fx["groups"]):
        _check_records(pop, rig, g, runs[gi, wave], "own+table", (gi, g["kind"]))
    # the other three choices of tables: on the publication groups and on one group of every other kind
    seen = set()
    for gi, g in enumerate(fx["groups"]):
        if g["kind"] != "publication" and g["kind"] in seen:
            continue
        seen.add(g["kind"])
        inp = rig.inputs(g)
        table = rig.sogm._dev(_bytes(pop, _records(pop, g["records"]), g["n_swarm"]), np.uint8)
        for mode in PUB_MODES[1:]:
            got = rig.run(inp, table, g["n_swarm"], wave, mode)
            assert got["ok"].tolist() == [e["ok"] for e in g["egos"]], (gi, mode)
            _check_records(pop, rig, g, got, mode, (gi, g["kind"], mode))
            if mode == "table":  # without an own table nothing is published: the next swarm table keeps what it held
                assert np.array_equal(got["table"], rig.prev["prev_table"][:len(g["egos"])]), (gi, mode)


@pytest.mark.gpu
def test_no_swarm_and_invalid_arguments(pop, fx, rig):
    """without a table every solved agent is safe, whatever n_swarm says (the grouped form then leaves out_safe alone, as
    sogm_replan's does); invalid arguments are reported"""
    g = next(g for g in fx["groups"] if g["kind"] == "publication" and g["egos"][0]["due"] is None)
    inp = rig.inputs(g)
    for wave in (False, True):
        got = rig.run(inp, None, 7, wave)
        assert got["ok"].tolist() == [e["solved"] for e in g["egos"]]
        assert got["safe"].tolist() == [1 if wave else -1] * len(g["egos"])
    lib, abi = pop.lib(), pop._abi
    p = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (
        ("planner", None), ("tau", C.c_double(0.3)), ("ret", p(inp["ret"])), ("npoly", p(inp["npoly"])),
        ("status", p(inp["status"])), ("cpts", p(inp["cpts"])), ("swarm", None), ("n_swarm", 0), ("ego", None),
        ("now", None), ("t_start", p(inp["t_start"])), ("ids", p(inp["ids"])), ("due", None), ("n", 0), ("out", None),
        ("ok", None), ("safe", None), ("own", None), ("table", None), ("flags", 0), ("stream", None))]
    assert lib.sogm_finish_batched(*args()) == abi.SOGM_OK                      # n = 0: nothing to do
    assert lib.sogm_finish_batched(*args(n=1)) == abi.SOGM_ERR_INVALID_ARG      # no outputs
    assert lib.sogm_finish_batched(*args(n_swarm=-1)) == abi.SOGM_ERR_INVALID_ARG
    assert lib.sogm_finish_batched(*args(flags=2)) == abi.SOGM_ERR_INVALID_ARG
    assert lib.sogm_finish_batched(*args(n=-1)) == abi.SOGM_ERR_INVALID_ARG
