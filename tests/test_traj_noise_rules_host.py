"""CPU: the message noise (include/sogm_abi.h "message noise") without a GPU.
  1. the rules of csrc/sogm_trajnoise.hpp, compiled with the host compiler (tests/traj_noise_rules_host_test.cpp), against
     the plain Python reading of the header (tests/traj_noise_reference.py): the known answers, keys and draws over a grid of
     (seed, tick, sender, loc_hold), whole records byte for byte with every n_pieces that takes another path, zero parameters
     on a record of special values, each sigma alone, the parameter refusals; the same program under
     -fsanitize=address,undefined runs them clean;
  2. the reading held to facts that do not come from it: the draws' mean and spread, the bias epochs;
  3. the entry refuses bad arguments before it looks for a device; parse_noise round trips."""
import ctypes as C
import math
import os
import shutil
import statistics
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traj_noise_reference as nref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5067
FULL = nref.params(SEED, (0.1, 0.05, 0.02), 0.05, 0.05, 3)
N_PIECES = (-1, 0, 1, 2, 15, 16, 17)


def bits(x):
    return f"{struct.unpack('<Q', struct.pack('<d', float(x)))[0]:016x}"


def prm_text(p):
    return f"{p.seed:x} {bits(p.sigma_loc[0])} {bits(p.sigma_loc[1])} {bits(p.sigma_loc[2])} {bits(p.sigma_time)} " \
           f"{bits(p.sigma_track)} {p.loc_hold}"


def make_row(j, n_pieces, special=False):
    """a record whose every double is distinct; special: -0.0, NaNs with payloads and infinities among its control points"""
    row = np.zeros((), nref.RECORD)
    row["drone_id"], row["n_pieces"] = j, n_pieces
    row["time_start"] = 12.5 + 0.1 * j
    row["duration"] = 0.25 + 0.125 * np.arange(16)
    row["cpts"] = np.sin(np.arange(240) * 0.37 + j) * 7.0
    if special:
        words = row["cpts"].view(np.uint64)
        words[0], words[1], words[2] = 0x8000000000000000, 0x7FF8000000000123, 0xFFF0000000000000      # -0.0, a NaN, -inf
        words[3], words[16], words[239] = 0x7FF0000000000000, 0x7FF4000000000001, 0x8000000000000000   # +inf, a signalling NaN
        row["time_start"] = -0.0
    return row


def words_of(row):
    return np.frombuffer(row.tobytes(), np.uint64)


def record_case(tag, p, m, j, row):
    out, shifts = nref.noise_table(p, m, np.array([row] * (j + 1)))      # row j of a table: the sender index is the row's
    line = f"{tag} {prm_text(p)} {m} {j} " + " ".join(f"{w:x}" for w in words_of(row)) + "\n"
    want = tag + "".join(f" {w:x}" for w in words_of(out[j])) + "".join(" " + bits(s) for s in shifts[j])
    return line, want, out[j]


def refused(p):
    return not all(math.isfinite(s) and s >= 0 for s in (*p.sigma_loc, p.sigma_time, p.sigma_track)) or p.loc_hold < 0


PARAM_CASES = [nref.params(), FULL, nref.params(1, (0, 0, 0), 0, 0, 7), nref.params(1, (-0.1, 0, 0)), nref.params(1, (0, 0, -1e-9)),
               nref.params(1, (0, float("nan"), 0)), nref.params(1, (0, 0, float("inf"))), nref.params(1, time=-1.0),
               nref.params(1, time=float("nan")), nref.params(1, track=float("inf")), nref.params(1, track=-0.5),
               nref.params(1, hold=-1)]


@pytest.fixture(scope="module")
def expected():
    lines, want = [], []
    for x in (0, 1, SEED, 2 ** 64 - 1):
        lines.append(f"M {x:x}\n")
        want.append(f"M {nref.mix(x):016x}")
    assert want[0] == "M e220a8397b1dcdaf"
    # the header's known answers, literally
    known = (((1, 0, 0), "4acd8eb1a9cfdcc6", ("0x1.469p-2", "-0x1.c25p-4", "-0x1.a0b6p-1")),
             ((2, 0, 3), "f86e1bf400ff8055", ("-0x1.1598p-1", None, None)),
             ((3, 7, 4), "0e12de2e62b1fc89", ("0x1.d6dep-1", "-0x1.34dep+0", "0x1.8a64p-1")))
    for (tag, x, j), k, ns in known:
        kk = nref.key(SEED, tag, x, j)
        assert f"{kk:016x}" == k
        for c, n in enumerate(ns):
            if n is not None:
                assert nref.draw(kk, c) == float.fromhex(n)
        lines.append(f"K {SEED:x} {tag:x} {x:x} {j:x}\n")
        want.append(f"K {k} " + " ".join(bits(float.fromhex(n)) if n is not None else bits(nref.draw(kk, c))
                                         for c, n in enumerate(ns)))
    # keys, draws and shifts over a grid
    for seed in (0, SEED, 2 ** 64 - 1):
        for m in (0, 1, 5, 2 ** 31 - 1):
            for j in (0, 1, 4, 129):
                for tag in (1, 2, 3):
                    lines.append(f"K {seed:x} {tag:x} {m:x} {j:x}\n")
                    k = nref.key(seed, tag, m, j)
                    want.append(f"K {k:016x} " + " ".join(bits(nref.draw(k, c)) for c in range(3)))
                for hold in (0, 1, 3):
                    p = FULL._replace(seed=seed, loc_hold=hold)
                    lines.append(f"H {prm_text(p)} {m} {j}\n")
                    want.append("H " + " ".join(bits(s) for s in nref.shift(p, m, j)))
    # whole records: every n_pieces that takes another path, out of place and in place
    alone = [nref.params(SEED, (0.1, 0, 0)), nref.params(SEED, (0, 0.1, 0)), nref.params(SEED, (0, 0, 0.1)),
             nref.params(SEED, time=0.05), nref.params(SEED, track=0.05)]
    for n in N_PIECES:
        for p in (FULL, nref.params(SEED)):
            for tag in "RI":
                line, w, _ = record_case(tag, p, 7, 4, make_row(4, n))
                lines.append(line)
                want.append(w)
    for p in alone:                                                     # each sigma alone
        line, w, out = record_case("R", p, 2, 1, make_row(1, 3))
        lines.append(line)
        want.append(w)
        moved = words_of(out) != words_of(make_row(1, 3))
        assert moved.any() and moved.sum() <= 45
    # zero parameters on a record that holds -0.0, NaN and +-inf: byte for byte
    for n in (3, 16):
        special = make_row(2, n, special=True)
        line, w, out = record_case("R", nref.params(SEED), 3, 2, special)
        assert out.tobytes() == special.tobytes()
        lines.append(line)
        want.append(w)
    for p in PARAM_CASES:
        lines.append(f"P {prm_text(p)}\n")
        want.append(f"P {int(refused(p))}")
    assert sum(w == "P 1" for w in want) == 9
    return "".join(lines), want


def _compile(tmp_path_factory, extra, tag):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("host compiler not available")
    out = str(tmp_path_factory.mktemp(tag) / "traj_noise_rules_host_test")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
           "-I", os.path.join(ROOT, "pred-occ-planner_amd", "csrc"),
           os.path.join(ROOT, "tests", "traj_noise_rules_host_test.cpp"), "-o", out]
    return cmd, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, [], "trajnoise")
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    cmd, out = _compile(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "trajnoise_san")
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
    bad = [(i, g[:200], w[:200]) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:3])
    kinds = {k: sum(1 for w in want if w.startswith(k)) for k in "MKHRIP"}
    print("lines per kind:", kinds)
    assert kinds["K"] > 100 and kinds["H"] > 100 and kinds["R"] + kinds["I"] >= 30


def test_host_rules_equal_the_reading(exe, tmp_path, expected):
    check_all(exe, tmp_path, expected)


def test_host_rules_run_clean_under_the_sanitizers(exe_sanitized, tmp_path, expected):
    check_all(exe_sanitized, tmp_path, expected)


# ---- 2. the reading held to facts that do not come from it ------------------------------------------------------------------
def test_the_draws_are_standard_normal():
    xs = [nref.draw(nref.key(SEED, nref.TAG_TRACK, m, j), c) for m in range(100) for j in range(32) for c in range(3)]
    mean, std = statistics.fmean(xs), statistics.pstdev(xs)
    print(len(xs), mean, std)
    assert len(xs) == 9600 and abs(mean) < 0.05 and abs(std - 1.0) < 0.05
    assert all(abs(x) <= 6.0 and x * 65536.0 == math.floor(x * 65536.0) for x in xs)      # a multiple of 2^-16 within +-6


def test_the_reading_moves_what_the_rule_says():
    row = make_row(4, 3)
    out, shifts = nref.noise_table(FULL, 7, np.array([row] * 5))
    s = shifts[4]
    assert all(v != 0.0 for v in s)
    assert np.array_equal(out["cpts"][4, :45], row["cpts"][:45] + np.tile(s[:3], 15))      # numpy's add is the same one add
    assert np.array_equal(out["cpts"][4, 45:], row["cpts"][45:]) and out["time_start"][4] == row["time_start"] + s[3]
    assert np.array_equal(out["duration"][4], row["duration"]) and out["n_pieces"][4] == 3 and out["drone_id"][4] == 4
    # an empty row is not a message; 17 pieces are noised as 16
    for n in (-1, 0):
        out, shifts = nref.noise_table(FULL, 7, np.array([make_row(0, n)]))
        assert out.tobytes() == make_row(0, n).tobytes() and not shifts.any()
    o16, _ = nref.noise_table(FULL, 7, np.array([make_row(0, 16)]))
    o17, _ = nref.noise_table(FULL, 7, np.array([make_row(0, 17)]))
    assert np.array_equal(o16["cpts"], o17["cpts"])
    # the clock offset is the sender's for the whole run, the tracking error is new with every message, the bias lasts
    # loc_hold ticks
    only_loc = nref.params(SEED, (0.1, 0.1, 0.1), hold=3)
    b = [nref.shift(only_loc, m, 2)[:3] for m in range(8)]
    assert [m for m in range(1, 8) if b[m] != b[m - 1]] == [3, 6]
    assert len({nref.shift(FULL, m, 2)[3] for m in range(8)}) == 1
    assert len({tuple(nref.shift(nref.params(SEED, track=0.05), m, 2)[:3]) for m in range(8)}) == 8
    assert len({tuple(nref.shift(nref.params(SEED, (0.1, 0.1, 0.1)), m, 2)) for m in range(8)}) == 1     # hold 0: the whole run


# ---- 3. the entry refuses bad arguments before it looks for a device --------------------------------------------------------
def test_entry_refuses_bad_arguments_first(pop):
    import torch
    abi, lib = pop._abi, pop.lib()
    assert abi.TRAJ_NOISE_BYTES == 56
    prm = abi.SogmTrajNoise()
    prm.seed, prm.sigma_time = 1, 0.5
    assert lib.sogm_traj_noise_default_params(C.byref(prm)) == abi.SOGM_OK
    assert bytes(prm) == bytes(56)                                               # all zero: no noise
    assert lib.sogm_traj_noise_default_params(None) == abi.SOGM_ERR_INVALID_ARG
    fake = 0x1000                                                                # never dereferenced: refused, or no device

    def noise(prm=prm, tick=0, table=fake, n_total=4, out=fake, shift=fake):
        return lib.sogm_traj_noise(C.byref(prm) if prm is not None else None, tick, table, n_total, out, shift, None)

    def with_prm(p):
        q = abi.SogmTrajNoise()
        q.seed, q.sigma_time, q.sigma_track, q.loc_hold = p.seed, p.sigma_time, p.sigma_track, p.loc_hold
        for c in range(3):
            q.sigma_loc[c] = p.sigma_loc[c]
        return q

    bad_prm = [with_prm(p) for p in PARAM_CASES if refused(p)]
    assert len(bad_prm) == 9
    bad = [lambda: noise(prm=None), lambda: noise(table=None), lambda: noise(out=None), lambda: noise(tick=-1),
           lambda: noise(n_total=0), lambda: noise(n_total=-3), lambda: noise(table=fake + 8), lambda: noise(out=fake + 4)]
    bad += [lambda p=p: noise(prm=p) for p in bad_prm]
    for i, call in enumerate(bad):
        assert call() == abi.SOGM_ERR_INVALID_ARG, i
        assert b"sogm_traj_noise: " in lib.sogm_last_error(), i
    if not torch.cuda.is_available():                                            # the arguments have passed: no device
        assert noise() == abi.SOGM_ERR_NO_DEVICE and b"no HIP device" in lib.sogm_last_error()
        assert noise(shift=None, out=fake) == abi.SOGM_ERR_NO_DEVICE            # out_shift is optional
        assert noise(prm=with_prm(FULL), tick=2 ** 31 - 1) == abi.SOGM_ERR_NO_DEVICE
        with pytest.raises(pop.SogmError):
            abi.check(noise(), "sogm_traj_noise")


def test_parse_noise_round_trips(pop):
    import importlib
    links = importlib.import_module("pred-occ-planner_amd.links")
    p = links.parse_noise("loc=0.1,time=0.05,track=0.025,hold=3,seed=0x5067")
    assert (p.seed, tuple(p.sigma_loc), p.sigma_time, p.sigma_track, p.loc_hold) == (0x5067, (0.1, 0.1, 0.1), 0.05, 0.025, 3)
    p = links.parse_noise("loc=0.1/0.2/0.05")
    assert (p.seed, tuple(p.sigma_loc), p.sigma_time, p.sigma_track, p.loc_hold) == (0, (0.1, 0.2, 0.05), 0.0, 0.0, 0)
    assert bytes(links.parse_noise("")) == bytes(56)
    q = links.make_noise(seed=9, loc=(0.1, 0.2, 0.05), time=0.5, track=0.25, hold=2)
    assert bytes(links.parse_noise(links.format_noise(q))) == bytes(q)
    assert bytes(links.parse_noise(links.format_noise(p))) == bytes(p)
    for text in ("jitter=3", "loc=0.1/0.2", "loc"):
        with pytest.raises(ValueError):
            links.parse_noise(text)
