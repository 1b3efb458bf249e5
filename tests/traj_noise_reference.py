"""A second reading of the message noise (include/sogm_abi.h "message noise"), written from the header's wording alone in plain
Python integers and floats: no shared code with csrc/sogm_trajnoise.hpp.  Python's float is IEEE binary64 and every
expression below is one operation at a time, so the results are the header's bits.  Records are numpy structured rows
(RECORD); only their bytes are moved, the arithmetic is Python's.
    shift(prm, tick, j)            -> [shift x, y, z, tau] of a message
    noise_table(prm, tick, table)  -> (the noisy table, out_shift [n][4])
Test infrastructure; not collected by pytest."""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
MAX_PIECES = 16
TAG_LOC, TAG_TIME, TAG_TRACK = 1, 2, 3
RECORD = np.dtype([("drone_id", "<i4"), ("n_pieces", "<i4"), ("time_start", "<f8"), ("duration", "<f8", (MAX_PIECES,)),
                   ("cpts", "<f8", (MAX_PIECES * 15,))])
assert RECORD.itemsize == 2064

Params = namedtuple("Params", "seed sigma_loc sigma_time sigma_track loc_hold")


def params(seed=0, loc=(0.0, 0.0, 0.0), time=0.0, track=0.0, hold=0):
    return Params(int(seed), tuple(float(v) for v in loc), float(time), float(track), int(hold))


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def normal(h):
    """the twelve-piece Irwin-Hall normal of "sensor noise": the 16-bit pieces of mix(h + 2), mix(h + 3), mix(h + 4)"""
    S = 0
    for k in (2, 3, 4):
        w = mix((h + k) & M64)
        for p in range(4):
            S += (w >> (16 * p)) & 0xFFFF
    return (float(S) - 393210.0) * 2.0 ** -16


def key(seed, tag, x, j):
    return mix(mix(mix(mix(seed & M64) ^ tag) ^ (x & M64)) ^ (j & M64))


def draw(k, c):
    return normal((k + 16 * c) & M64)


def epoch(prm, m):
    return m // prm.loc_hold if prm.loc_hold > 0 else 0


def shift(prm, m, j):
    """[shift x, y, z, tau] of message (m, j)"""
    kb, ke = key(prm.seed, TAG_LOC, epoch(prm, m), j), key(prm.seed, TAG_TRACK, m, j)
    out = []
    for c in range(3):
        b = prm.sigma_loc[c] * draw(kb, c)
        e = prm.sigma_track * draw(ke, c)
        out.append(b + e)
    out.append(prm.sigma_time * draw(key(prm.seed, TAG_TIME, 0, j), 0))
    return out


def noise_table(prm, tick, table):
    """table: RECORD [n] -> (noisy RECORD [n], out_shift float64 [n][4])"""
    table = np.asarray(table).view(RECORD).reshape(-1)
    out = table.copy()
    shifts = np.zeros((table.shape[0], 4), np.float64)
    for j in range(table.shape[0]):
        n = int(table["n_pieces"][j])
        if n <= 0:
            continue
        s = shift(prm, tick, j)
        shifts[j] = s
        for i in range(15 * min(n, MAX_PIECES)):
            if s[i % 3] != 0.0:
                out["cpts"][j, i] = float(table["cpts"][j, i]) + s[i % 3]
        if s[3] != 0.0:
            out["time_start"][j] = float(table["time_start"][j]) + s[3]
    return out, shifts
