"""GPU: sogm_traj_noise (csrc/sogm_trajnoise.hip) against the plain Python reading of the header
(tests/traj_noise_reference.py), byte for byte, out_shift included.  n_total 1, 5 and 130 (more rows than a workgroup's four,
a ragged tail); rows mix n_pieces 0, 1, 3 and 16 — the odd ones put a noised and a copied double into one 16-byte piece, 16
reaches the record's last, lone 129th piece."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traj_noise_reference as nref  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5067
FULL = nref.params(SEED, (0.1, 0.05, 0.02), 0.05, 0.05, 3)
PIECES = (3, 0, 1, 16, 2, -1, 15, 17)


@pytest.fixture(scope="module")
def links(pop):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("pred-occ-planner_amd.links")


def make_table(n_total, raw=False):
    """every row has bytes of its own; unless raw, the doubles that take noise are finite (the rest stay arbitrary bits)"""
    rng = np.random.default_rng(SEED + n_total)
    t = np.zeros(n_total, nref.RECORD)
    t.view(np.uint8).reshape(n_total, 2064)[:] = rng.integers(0, 256, (n_total, 2064), dtype=np.uint8)
    for j in range(n_total):
        t[j]["drone_id"], t[j]["n_pieces"] = j, PIECES[j % len(PIECES)]
        if not raw:
            k = 15 * min(max(int(t[j]["n_pieces"]), 0), 16)
            t[j]["cpts"][:k] = rng.uniform(-20.0, 20.0, k)
            t[j]["time_start"] = 100.0 + 0.1 * j
    return t


def to_noise(links, p):
    return links.make_noise(p.seed, p.sigma_loc, p.sigma_time, p.sigma_track, p.loc_hold)


def on_device(table):
    import torch
    return torch.from_numpy(table.view(np.uint8).reshape(-1, 2064).copy()).cuda()


def run(links, p, tick, table, in_place=False):
    import torch
    dev = on_device(table)
    shift = torch.full((len(table), 4), 7.0, dtype=torch.float64, device="cuda")
    out = links.traj_noise(to_noise(links, p), tick, dev, dev if in_place else None, shift)
    torch.cuda.synchronize()
    if not in_place:
        assert dev.cpu().numpy().tobytes() == table.tobytes()                # the table is only read
    return out.cpu().numpy().tobytes(), shift.cpu().numpy()


@pytest.mark.parametrize("n_total", [1, 5, 130])
def test_kernel_equals_the_reading(links, n_total):
    table = make_table(n_total)
    for tick in (0, 7):
        want, want_shift = nref.noise_table(FULL, tick, table)
        got, got_shift = run(links, FULL, tick, table)
        assert got_shift.tobytes() == want_shift.tobytes()
        bad = [j for j in range(n_total) if got[j * 2064:(j + 1) * 2064] != want[j].tobytes()]
        assert not bad, bad[:5]
        again, again_shift = run(links, FULL, tick, table)                   # the same call twice: the same bytes
        assert again == got and again_shift.tobytes() == got_shift.tobytes()
        inp, inp_shift = run(links, FULL, tick, table, in_place=True)        # out == table
        assert inp == got and inp_shift.tobytes() == got_shift.tobytes()
    moved = sum(want[j].tobytes() != table[j].tobytes() for j in range(n_total))
    assert moved == sum(int(n) > 0 for n in table["n_pieces"])


def test_zero_parameters_copy_byte_for_byte(links):
    import torch
    table = make_table(130, raw=True)                                        # arbitrary bits: NaNs of every kind, -0.0, inf
    table[0]["cpts"][:4] = [-0.0, float("nan"), float("inf"), -float("inf")]
    got, shift = run(links, nref.params(SEED), 5, table)
    assert got == table.tobytes() and not shift.any()
    dev = on_device(table)                                                   # out_shift is optional
    out = links.traj_noise(links.make_noise(), 0, dev)
    assert torch.equal(out, dev)


@pytest.mark.parametrize("which", ["x", "y", "z", "time", "track"])
def test_each_sigma_alone(links, which):
    p = {"x": nref.params(SEED, (0.1, 0, 0)), "y": nref.params(SEED, (0, 0.1, 0)), "z": nref.params(SEED, (0, 0, 0.1)),
         "time": nref.params(SEED, time=0.05), "track": nref.params(SEED, track=0.05)}[which]
    table = make_table(9)
    want, want_shift = nref.noise_table(p, 4, table)
    got, got_shift = run(links, p, 4, table)
    assert got == want.tobytes() and got_shift.tobytes() == want_shift.tobytes()
    nz = {"x": [0], "y": [1], "z": [2], "time": [3], "track": [0, 1, 2]}[which]
    live = table["n_pieces"] > 0
    assert (got_shift[live][:, nz] != 0).all() and not np.delete(got_shift, nz, axis=1).any() and not got_shift[~live].any()


def test_the_bias_changes_when_its_hold_runs_out(links):
    p = nref.params(SEED, (0.1, 0.1, 0.1), hold=3)
    table = make_table(5)
    shifts = [run(links, p, tick, table)[1] for tick in range(8)]
    for tick in range(8):
        assert shifts[tick].tobytes() == nref.noise_table(p, tick, table)[1].tobytes()
    live = table["n_pieces"] > 0
    changed = [tick for tick in range(1, 8) if (shifts[tick][live] != shifts[tick - 1][live]).any()]
    assert changed == [3, 6]
