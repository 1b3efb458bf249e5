"""A second reading of the radio-link model (include/sogm_abi.h "radio links"), written from the header's wording alone in
plain Python integers and floats: no numpy arithmetic, no shared code with csrc/sogm_link.hpp.  Python's float is IEEE
binary64 and every expression below is one operation at a time, so the results are the header's bits.

A table is a list (or structured array) of rows; only `n_pieces` of a row is looked at, and rows are copied whole.
    LinkReading(n_total, agent0, n_local, prm).deliver(tick, table, pos) -> what the tick did, pair by pair
    .views[a_local][j]  the row held (None: nothing heard yet)      .held[a_local][j]  its send tick (-1)
    .counters[a_local]  the eight sums of the header
"""
import math
from collections import namedtuple

M64 = (1 << 64) - 1
MAX_DELAY = 7
NEWEST_WINS = 1
COUNTERS = ("sent", "out_of_range", "lost", "arrivals", "applied", "stale", "age_sum", "unheard")

Params = namedtuple("Params", "seed p_loss range delay_min delay_max flags")


def params(seed=0, p_loss=0.0, range=0.0, delay_min=0, delay_max=0, flags=0):
    return Params(int(seed), float(p_loss), float(range), int(delay_min), int(delay_max), int(flags))


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniform(w):
    return float(w >> 11) * 2.0 ** -53          # (w >> 11) < 2^53: the conversion is exact


def key(seed, m, j, a, n_total):
    return mix(mix(mix(seed & M64) ^ (m & M64)) ^ ((j * n_total + a) & M64))


def loss_draw(h):
    return uniform(mix(h & M64))


def delay_draw(prm, h):
    span = prm.delay_max - prm.delay_min + 1
    return prm.delay_min + min(int(math.floor(uniform(mix((h + 1) & M64)) * float(span))), span - 1)


def out_of_range(prm, pj, pa):
    if not prm.range > 0:
        return False
    dx, dy, dz = pj[0] - pa[0], pj[1] - pa[1], pj[2] - pa[2]
    d2 = (dx * dx + dy * dy) + dz * dz
    return not (d2 <= prm.range * prm.range)


# one message's fate: (exists, out of range, lost by draw, delay)
def message(prm, n_total, m, j, a, n_pieces, pj, pa):
    if n_pieces <= 0:
        return False, False, False, 0
    h = key(prm.seed, m, j, a, n_total)
    if out_of_range(prm, pj, pa):
        return True, True, False, delay_draw(prm, h)
    return True, False, loss_draw(h) < prm.p_loss, delay_draw(prm, h)


def n_pieces_of(row):
    try:
        return int(row["n_pieces"])
    except (TypeError, IndexError, KeyError, ValueError):
        return int(row.n_pieces)


class LinkReading:
    def __init__(self, n_total, agent0, n_local, prm):
        assert 0 <= prm.delay_min <= prm.delay_max <= MAX_DELAY and 0.0 <= prm.p_loss <= 1.0 and prm.range >= 0.0
        assert n_total >= 1 and 0 <= agent0 and 1 <= n_local <= n_total - agent0
        self.n_total, self.agent0, self.n_local, self.prm = n_total, agent0, n_local, prm
        self.sent = {}                                       # tick -> (rows, positions)
        self.tick0 = None
        self.views = [[None] * n_total for _ in range(n_local)]
        self.held = [[-1] * n_total for _ in range(n_local)]
        self.counters = [[0] * 8 for _ in range(n_local)]
        self.multi = self.silent = 0                         # pair-ticks with more than one arrival / with none

    def deliver(self, k, table, pos=None):
        prm, N = self.prm, self.n_total
        if self.tick0 is None:
            self.tick0 = k
        assert k == self.tick0 or k - 1 in self.sent, "ticks are consecutive"
        assert pos is not None or not prm.range > 0
        rows = [table[j] for j in range(N)]
        self.sent[k] = (rows, None if pos is None else [[float(pos[j][c]) for c in range(3)] for j in range(N)])
        self.sent.pop(k - MAX_DELAY - 1, None)
        log = []
        for al in range(self.n_local):
            a, c = self.agent0 + al, self.counters[al]
            for j in range(N):
                if j == a:
                    self.views[al][a], self.held[al][a] = rows[a], k
                    continue
                arrived = []
                for m in range(max(self.tick0, k - prm.delay_max), k + 1):
                    rs, ps = self.sent[m]
                    exists, far, lost, d = message(prm, N, m, j, a, n_pieces_of(rs[j]), ps[j] if ps else None,
                                                   ps[a] if ps else None)
                    if m == k and exists:
                        c[0] += 1
                        c[1] += far
                        c[2] += lost
                    if exists and not far and not lost and m + d == k:
                        arrived.append(m)
                c[3] += len(arrived)
                self.multi += len(arrived) > 1
                self.silent += not arrived
                if arrived:
                    m = max(arrived)
                    stale = m < self.held[al][j]
                    c[5] += stale
                    if not (stale and prm.flags & NEWEST_WINS):
                        self.views[al][j], self.held[al][j] = self.sent[m][0][j], m
                        c[4] += 1
                log.append((a, j, tuple(arrived)))
                if self.held[al][j] >= 0:
                    c[6] += k - self.held[al][j]
                else:
                    c[7] += 1
        return log

    def totals(self):
        return [sum(c[i] for c in self.counters) for i in range(8)]
