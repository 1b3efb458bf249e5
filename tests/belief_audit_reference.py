"""A second reading of the belief audit (include/sogm_abi.h "belief audit"), written from the header's wording alone in plain
Python integers and floats, one operation at a time: no shared code with csrc/sogm_belief.hpp.  Records are numpy structured
rows (traj_noise_reference.RECORD); the arithmetic is Python's.
    position(row, t)                                  -> [x, y, z] of a record at absolute time t, or None (no trajectory)
    audit(prm, truth, views, t_now, n_total, agent0)  -> (counters [n_local][12], pair_q [n_local][n_total])
Test infrastructure; not collected by pytest."""
import math
from collections import namedtuple

import numpy as np

MAX_PIECES = 16
COUNTERS = ("compared", "unheard", "phantom", "samples", "bin0", "bin1", "bin2", "bin3", "bin4", "bin5", "sum_q", "max_q")
Q_MAX = 1 << 40
A = ((1, -4, 6, -4, 1), (0, 4, -12, 12, -4), (0, 0, 6, -12, 6), (0, 0, 0, 4, -4), (0, 0, 0, 0, 1))

Params = namedtuple("Params", "dt_sample edges n_samples")


def params(dt_sample=0.2, edges=(0.05, 0.1, 0.2, 0.5, 1.0), n_samples=8):
    return Params(float(dt_sample), tuple(float(e) for e in edges), int(n_samples))


def position(row, t_abs):
    n = min(int(row["n_pieces"]), MAX_PIECES)
    if n <= 0:
        return None
    dur = [float(d) for d in row["duration"][:n]]
    tt = t_abs - float(row["time_start"])
    total = 0.0
    for d in dur:
        total = total + d
    tt = 0.0 if tt < 0 else (total if tt > total else tt)
    piece, rem = n - 1, tt
    for k in range(n):
        rem = rem - dur[k]
        if rem < 0:
            piece = k
            break
    t0 = 0.0
    for k in range(piece):
        t0 = t0 + dur[k]
    tf = t0 + dur[piece]
    span = tf - t0
    num = tt - t0
    with np.errstate(all="ignore"):
        s = float(np.float64(num) / np.float64(span))       # one IEEE division (Python's own raises on a zero span)
    s2 = s * s
    S0 = (1.0, s, s2, s2 * s, s2 * s2)
    c = row["cpts"][piece * 15:piece * 15 + 15]
    out = []
    for d in range(3):
        p = 0.0
        for j in range(5):
            b = 0.0
            for q in range(5):
                b = b + float(c[q * 3 + d]) * float(A[q][j])
            p = p + b * S0[j]
        out.append(p)
    return out


def sample(prm, pT, pB):
    """(bin, q) of one compared sample"""
    dx, dy, dz = pB[0] - pT[0], pB[1] - pT[1], pB[2] - pT[2]
    d2 = (dx * dx + dy * dy) + dz * dz
    b = 5
    for i in range(5):
        if d2 <= prm.edges[i] * prm.edges[i]:
            b = i
            break
    y = d2 * 1e6 + 0.5
    q = Q_MAX if (y != y or y >= float(Q_MAX)) else min(int(math.floor(y)), Q_MAX)
    return b, q, d2


def audit(prm, truth, views, t_now, n_total, agent0, n_local, on_sample=None):
    counters = [[0] * 12 for _ in range(n_local)]
    pair_q = [[-1] * n_total for _ in range(n_local)]
    for al in range(n_local):
        a, c = agent0 + al, counters[al]
        for j in range(n_total):
            if j == a:
                continue
            T, B = truth[j], views[al][j]
            hasT, hasB = int(T["n_pieces"]) > 0, int(B["n_pieces"]) > 0
            if not hasT and not hasB:
                continue
            if hasT and not hasB:
                c[1] += 1
                continue
            if hasB and not hasT:
                c[2] += 1
                continue
            c[0] += 1
            worst = 0
            for s in range(prm.n_samples):
                t = float(t_now[al]) + float(s) * prm.dt_sample
                b, q, d2 = sample(prm, position(T, t), position(B, t))
                if on_sample is not None:
                    on_sample(d2)
                c[3] += 1
                c[4 + b] += 1
                c[10] += q
                worst = max(worst, q)
            c[11] = max(c[11], worst)
            pair_q[al][j] = worst
    return np.array(counters, np.int64), np.array(pair_q, np.int64)
