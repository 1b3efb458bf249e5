"""CPU: the radio-link model (include/sogm_abi.h "radio links") without a GPU.
  1. the rules of csrc/sogm_link.hpp, compiled with the host compiler (tests/link_rules_host_test.cpp), against the plain
     Python reading of the header (tests/link_model_reference.py): the known answers, keys and draws over a grid of messages,
     the range test at its edges, the parameter refusals, and whole runs pair by pair and tick by tick — the 5-agent,
     12-tick case of the header with and without SOGM_LINK_NEWEST_WINS, a shard, a range, empty rows, the longest delay;
     the same program under -fsanitize=address,undefined runs them clean;
  2. the reading held to the header's counts;
  3. the three entries refuse bad arguments before they look for a device."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_model_reference as lref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5067
HEADER = lref.params(SEED, 0.3, 0.0, 0, 2)          # the header's case: n_total 5, ticks 0 .. 11


class Row:
    def __init__(self, n_pieces):
        self.n_pieces = n_pieces


def bits(x):
    return f"{struct.unpack('<Q', struct.pack('<d', float(x)))[0]:016x}"


def next_up(x):
    return struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", x))[0] + 1))[0]


def positions(n_total, k):
    """agents on a slowly opening line: pairs drift through a 2.5 m range; agent 3 has no position fix at tick 4"""
    pos = [[0.9 * j + 0.07 * k * j, 0.3 * ((j * 7 + k) % 3), 1.0 + 0.1 * j] for j in range(n_total)]
    if k == 4 and n_total > 3:
        pos[3][1] = float("nan")
    return pos


def pieces(n_total, k, holes):
    """row j is empty at the ticks `holes` names for it"""
    return [0 if (j, k) in holes else 3 for j in range(n_total)]


def run_case(prm, n_total, agent0, n_local, tick0, n_ticks, with_pos=False, holes=()):
    """(the program's input for one S case, the reading's answer line by line, the reading)"""
    head = (f"S {prm.seed:x} {bits(prm.p_loss)} {bits(prm.range)} {prm.delay_min} {prm.delay_max} {prm.flags} "
            f"{n_total} {agent0} {n_local} {tick0} {n_ticks} {int(with_pos)}")
    lines, want = [head], []
    r = lref.LinkReading(n_total, agent0, n_local, prm)
    for k in range(tick0, tick0 + n_ticks):
        n = pieces(n_total, k, holes)
        pos = positions(n_total, k) if with_pos else None
        lines.append(" ".join(str(v) for v in n))
        if with_pos:
            lines.append(" ".join(bits(c) for p in pos for c in p))
        log = {(a, j): arr for a, j, arr in r.deliver(k, [Row(v) for v in n], pos)}
        for al in range(n_local):
            a = agent0 + al
            for j in range(n_total):
                if j != a:
                    mask = sum(1 << (k - m) for m in log[(a, j)])
                    want.append(f"V {k} {a} {j} {r.held[al][j]} {mask:x}")
            want.append(f"C {k} {a} " + " ".join(str(c) for c in r.counters[al]))
    return "\n".join(lines) + "\n", want, r


SWARM_CASES = (
    dict(prm=HEADER, n_total=5, agent0=0, n_local=5, tick0=0, n_ticks=12),
    dict(prm=HEADER._replace(flags=lref.NEWEST_WINS), n_total=5, agent0=0, n_local=5, tick0=0, n_ticks=12),
    dict(prm=HEADER, n_total=5, agent0=1, n_local=3, tick0=0, n_ticks=12),                            # a shard
    dict(prm=lref.params(SEED, 0.2, 2.5, 0, 3), n_total=6, agent0=0, n_local=6, tick0=3, n_ticks=14, with_pos=True,
         holes={(2, 3), (2, 4), (2, 5), (4, 9), (0, 16)}),                                            # range, NaN, empty rows
    dict(prm=lref.params(SEED + 1, 0.1, 0.0, 0, 7), n_total=4, agent0=0, n_local=4, tick0=0, n_ticks=20),   # the ring wraps
    dict(prm=lref.params(SEED, 0.0, 0.0, 7, 7), n_total=3, agent0=0, n_local=3, tick0=5, n_ticks=10),
    dict(prm=lref.params(SEED, 1.0, 0.0, 0, 2), n_total=3, agent0=0, n_local=3, tick0=0, n_ticks=4),
    dict(prm=lref.params(), n_total=3, agent0=0, n_local=3, tick0=0, n_ticks=3),                      # perfect links
)


def refused(p_loss, rng, dmin, dmax):
    return not (math.isfinite(p_loss) and 0.0 <= p_loss <= 1.0 and math.isfinite(rng) and rng >= 0.0
                and 0 <= dmin <= dmax <= lref.MAX_DELAY)


PARAM_CASES = [(0.0, 0.0, 0, 0), (1.0, 5.0, 0, 7), (0.5, 0.0, 7, 7), (-0.1, 0.0, 0, 0), (1.5, 0.0, 0, 0),
               (float("nan"), 0.0, 0, 0), (0.0, -1.0, 0, 0), (0.0, float("inf"), 0, 0), (0.0, float("nan"), 0, 0),
               (0.0, 0.0, -1, 0), (0.0, 0.0, 2, 1), (0.0, 0.0, 0, 8), (float("inf"), 0.0, 0, 0)]


@pytest.fixture(scope="module")
def expected():
    lines, want = [], []
    for x in (0, 1, SEED, 2 ** 64 - 1):
        lines.append(f"M {x:x}\n")
        want.append(f"M {lref.mix(x):016x}")
    assert want[0] == "M e220a8397b1dcdaf"
    # the header's known answers, literally
    known = (((0, 0, 1), "f556f0f326877456", "0x1.570a43181f084p-3", 0, 1),
             ((3, 1, 2), "e38b8086c8cb24dd", "0x1.18add1ad9b2b0p-3", 0, 1),
             ((7, 4, 0), "eceed24989f9f5f8", "0x1.5e11450a71e6bp-1", 1, 0))
    for (m, j, a), h, u, d, lost in known:
        lines.append(f"K {SEED:x} {m} {j} {a} 5 {bits(0.3)} 0 2\n")
        want.append(f"K {h} {bits(float.fromhex(u))} {d} {lost}")
        hh = lref.key(SEED, m, j, a, 5)
        assert (f"{hh:016x}", lref.loss_draw(hh), lref.delay_draw(HEADER, hh)) == (h, float.fromhex(u), d)
    for prm, n_total in ((HEADER, 5), (lref.params(2 ** 64 - 1, 0.5, 0.0, 1, 7), 128), (lref.params(9, 0.9, 0.0, 3, 3), 7)):
        for m in (0, 1, 17, 2 ** 31 - 1):
            for j in range(0, n_total, max(1, n_total // 5)):
                for a in range(0, n_total, max(1, n_total // 4)):
                    lines.append(f"K {prm.seed:x} {m} {j} {a} {n_total} {bits(prm.p_loss)} {prm.delay_min} {prm.delay_max}\n")
                    h = lref.key(prm.seed, m, j, a, n_total)
                    u = lref.loss_draw(h)
                    want.append(f"K {h:016x} {bits(u)} {lref.delay_draw(prm, h)} {int(u < prm.p_loss)}")
    # the range test at its edges: d2 == range^2 is in range, the next double up is out; a NaN is out; range 0 never is
    r = 2.5
    edge = math.sqrt(r * r - 1.5 * 1.5)                      # (1.5, 2.0, 0): 2.25 + 4.0 == 6.25 exactly
    assert edge == 2.0
    dj = (2.5 - 0.0, 0.0, (1.0 + 2.0 ** -25) - 1.0)          # d2 is the double after range^2, exactly
    assert (dj[0] * dj[0] + dj[1] * dj[1]) + dj[2] * dj[2] == next_up(r * r)
    for rng, pj, pa in ((r, (1.5, 2.0, 0.0), (0.0, 0.0, 0.0)), (r, (1.5, next_up(2.0), 0.0), (0.0, 0.0, 0.0)),
                        (r, (2.5, 0.0, 1.0 + 2.0 ** -25), (0.0, 0.0, 1.0)),
                        (r, (0.0, 0.0, r), (0.0, 0.0, 0.0)), (r, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0 + next_up(r))),
                        (r, (float("nan"), 0.0, 0.0), (0.0, 0.0, 0.0)), (r, (0.0, 0.0, 0.0), (0.0, float("nan"), 0.0)),
                        (r, (float("inf"), 0.0, 0.0), (float("inf"), 0.0, 0.0)), (0.0, (1e9, 0.0, 0.0), (0.0, 0.0, 0.0)),
                        (0.0, (float("nan"), 0.0, 0.0), (0.0, 0.0, 0.0)), (1e-3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))):
        lines.append("G " + " ".join(bits(v) for v in (rng, *pj, *pa)) + "\n")
        want.append(f"G {int(lref.out_of_range(lref.params(range=rng), pj, pa))}")
    assert [w for w in want if w.startswith("G")] == ["G 0", "G 1", "G 1", "G 0", "G 1", "G 1", "G 1", "G 1", "G 0", "G 0", "G 0"]
    for p_loss, rng, dmin, dmax in PARAM_CASES:
        lines.append(f"P {bits(p_loss)} {bits(rng)} {dmin} {dmax}\n")
        want.append(f"P {int(refused(p_loss, rng, dmin, dmax))}")
    for case in SWARM_CASES:
        text, w, _ = run_case(**case)
        lines.append(text)
        want += w
    return "".join(lines), want


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "link_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "link_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "link")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "link_san")
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
    kinds = {k: sum(1 for w in want if w.startswith(k)) for k in ("M", "K", "G", "P", "V", "C")}
    print("lines per kind:", kinds)
    assert kinds["K"] > 100 and kinds["V"] > 1000 and kinds["C"] > 200


def test_host_rules_equal_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_rules_run_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


# ---- 2. the reading held to the header's counts -----------------------------------------------------------------------------
def header_run(prm, n_total=5, n_ticks=12):
    r = lref.LinkReading(n_total, 0, n_total, prm)
    unheard_last = None
    for k in range(n_ticks):
        before = r.totals()[7]
        r.deliver(k, [Row(3)] * n_total)
        unheard_last = r.totals()[7] - before
    return r, dict(zip(lref.COUNTERS, r.totals())), unheard_last


def test_the_reading_reproduces_the_headers_counts():
    r, c, unheard_last = header_run(HEADER)
    print(c, "multi", r.multi, "silent", r.silent)
    assert (c["sent"], c["out_of_range"], c["lost"], c["arrivals"], c["stale"]) == (240, 0, 79, 147, 7)
    assert (r.multi, r.silent) == (25, 121)
    assert unheard_last == 0 and all(h >= 0 for row in r.held for h in row)      # every sender heard by tick 11
    assert c["applied"] == 12 * 20 - r.silent                                    # every pair-tick with an arrival applies one


def test_newest_wins_drops_the_stale_arrivals():
    plain, c0, _ = header_run(HEADER)
    r, c, _ = header_run(HEADER._replace(flags=lref.NEWEST_WINS))
    assert (c["sent"], c["lost"], c["arrivals"], c["stale"]) == (240, 79, 147, 7)
    assert c["applied"] == c0["applied"] - 7
    assert c["age_sum"] < c0["age_sum"]                                          # the views are fresher for it
    # under the flag a held tick never goes back
    r2, prev = lref.LinkReading(5, 0, 5, HEADER._replace(flags=lref.NEWEST_WINS)), None
    went_back = 0
    p2 = lref.LinkReading(5, 0, 5, HEADER)
    prev_plain = None
    for k in range(12):
        r2.deliver(k, [Row(3)] * 5)
        p2.deliver(k, [Row(3)] * 5)
        now, now_plain = [list(h) for h in r2.held], [list(h) for h in p2.held]
        if prev is not None:
            assert all(n >= p for rn, rp in zip(now, prev) for n, p in zip(rn, rp))
            went_back += sum(n < p for rn, rp in zip(now_plain, prev_plain) for n, p in zip(rn, rp))
        prev, prev_plain = now, now_plain
    assert went_back == 7


def test_perfect_and_uniformly_late_links():
    _, c, _ = header_run(lref.params(SEED, 0.0, 0.0, 0, 0))
    assert (c["sent"], c["arrivals"], c["applied"], c["stale"], c["age_sum"], c["unheard"]) == (240, 240, 240, 0, 0, 0)
    _, c, _ = header_run(lref.params(SEED, 0.0, 0.0, 1, 1))
    assert (c["sent"], c["arrivals"], c["stale"], c["unheard"]) == (240, 220, 0, 20)
    assert c["age_sum"] == 220                                                   # every view is exactly one tick old


def test_total_loss_hears_nothing():
    r, c, _ = header_run(lref.params(SEED, 1.0, 0.0, 0, 2))
    assert (c["sent"], c["lost"], c["arrivals"], c["unheard"]) == (240, 240, 0, 240)
    assert all(r.views[a][j] is None for a in range(5) for j in range(5) if j != a)
    assert all(r.views[a][a] is not None for a in range(5))                      # but its own row


def test_the_range_case_takes_its_branches():
    _, _, r = run_case(**SWARM_CASES[3])
    c = dict(zip(lref.COUNTERS, r.totals()))
    print(c, r.multi, r.silent)
    assert c["out_of_range"] > 20 and c["lost"] > 20 and c["stale"] > 0 and r.multi > 0 and c["unheard"] > 0
    assert c["sent"] < 14 * 30 and c["sent"] - c["out_of_range"] - c["lost"] >= c["arrivals"] > 50


# ---- 3. the entries refuse bad arguments before they look for a device ------------------------------------------------------
def test_entries_refuse_bad_arguments_first(pop):
    import torch
    abi, lib = pop._abi, pop.lib()
    assert abi.LINK_PARAMS_BYTES == 40 and C.sizeof(abi.SogmLinkBuffers) == 40
    prm = abi.SogmLinkParams()
    prm.seed, prm.p_loss = 1, 0.5
    assert lib.sogm_link_default_params(C.byref(prm)) == abi.SOGM_OK
    assert bytes(prm) == bytes(40)                                               # all zero: perfect links
    assert lib.sogm_link_default_params(None) == abi.SOGM_ERR_INVALID_ARG
    fake = 0x1000                                                                # never dereferenced: refused, or no device
    buf = abi.SogmLinkBuffers(fake, fake, fake, fake, fake)

    def deliver(prm=prm, tick=0, tick0=0, table=fake, pos=fake, n_total=4, agent0=0, n_local=4, b=buf):
        return lib.sogm_link_deliver(C.byref(prm) if prm is not None else None, tick, tick0, table, pos, n_total, agent0,
                                     n_local, C.byref(b) if b is not None else None, None)

    def init(prm=prm, n_total=4, n_local=4, b=buf):
        return lib.sogm_link_init(C.byref(prm) if prm is not None else None, n_total, n_local,
                                  C.byref(b) if b is not None else None, None)

    def with_prm(**kw):
        p = abi.SogmLinkParams()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad_prm = [with_prm(p_loss=p, range=r, delay_min=lo, delay_max=hi) for p, r, lo, hi in PARAM_CASES if refused(p, r, lo, hi)]
    assert len(bad_prm) >= 9
    ranged = with_prm(range=2.0)
    no_ring_pos = abi.SogmLinkBuffers(fake, None, fake, fake, fake)
    bad = [lambda: deliver(prm=None), lambda: deliver(b=None), lambda: deliver(table=None),
           lambda: deliver(prm=ranged, pos=None), lambda: deliver(prm=ranged, b=no_ring_pos),
           lambda: deliver(tick=2, tick0=3), lambda: deliver(tick0=-1, tick=-1), lambda: deliver(n_total=0),
           lambda: deliver(agent0=-1), lambda: deliver(n_local=0), lambda: deliver(agent0=2, n_local=3),
           lambda: deliver(b=abi.SogmLinkBuffers(fake + 8, fake, fake, fake, fake)),
           lambda: init(prm=None), lambda: init(b=None), lambda: init(n_total=0), lambda: init(n_local=5),
           lambda: init(prm=ranged, b=no_ring_pos)]
    bad += [lambda p=p: deliver(prm=p) for p in bad_prm] + [lambda p=p: init(prm=p) for p in bad_prm]
    for i, field in enumerate(("ring_table", "views", "held_tick", "counters")):
        b = abi.SogmLinkBuffers(fake, fake, fake, fake, fake)
        setattr(b, field, None)
        bad += [lambda b=b: deliver(b=b), lambda b=b: init(b=b)]
    for i, call in enumerate(bad):
        assert call() == abi.SOGM_ERR_INVALID_ARG, i
        assert b"sogm_link_" in lib.sogm_last_error(), i
    if not torch.cuda.is_available():                                            # the arguments have passed: no device
        assert deliver() == abi.SOGM_ERR_NO_DEVICE and b"no HIP device" in lib.sogm_last_error()
        assert deliver(pos=None) == abi.SOGM_ERR_NO_DEVICE                       # no range: no positions needed
        assert deliver(b=no_ring_pos, pos=None) == abi.SOGM_ERR_NO_DEVICE
        assert init() == abi.SOGM_ERR_NO_DEVICE
        with pytest.raises(pop.SogmError):
            abi.check(init(), "sogm_link_init")


def test_parse_params(pop):
    import importlib
    links = importlib.import_module("pred-occ-planner_amd.links")
    p = links.parse_params("loss=0.3,delay=0..2,range=12.5,seed=0x5067,newest")
    assert (p.seed, p.p_loss, p.range, p.delay_min, p.delay_max, p.flags) == (0x5067, 0.3, 12.5, 0, 2, 1)
    p = links.parse_params("delay=1")
    assert (p.seed, p.p_loss, p.range, p.delay_min, p.delay_max, p.flags) == (0, 0.0, 0.0, 1, 1, 0)
    assert bytes(links.parse_params("")) == bytes(40)
    with pytest.raises(ValueError):
        links.parse_params("jitter=3")
