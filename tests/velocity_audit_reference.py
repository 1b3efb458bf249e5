"""A numpy reading of include/sogm_abi.h "velocity audit", written from the definition's text and not from
csrc/sogm_velaudit.hpp: one agent's new-born list, its source index and the truth arrays of its input points -> the 32-value
row and the per-code table.  Sequential on purpose: one point at a time, fp32 one operation at a time (np.float32 scalars)."""
import numpy as np

ROW = 32
STATIC, TRACKED, UNTRACKED, DROPPED = 0, 1, 2, 3
STILL, MOVING = 0, 1
SKIPPED, BAD_SOURCE, CLIPPED = 1, 2, 4
HIT_GROUND = -1
THRESHOLDS = [np.float32(t) for t in (0.1, 0.25, 0.5, 1.0, 2.0)]
COS2_15 = np.float32(0.9330127)
F = np.float32


def estimate_class(vx, inten):
    if not (F(inten) > F(0.01)):
        return STATIC
    return TRACKED if F(vx) > F(-100.0) else UNTRACKED


def truth_class(inten):
    return MOVING if F(inten) > F(0.01) else STILL


def code_row(code, n_codes):
    code = int(code)
    if 0 <= code < n_codes:
        return code
    return n_codes if code == HIT_GROUND else n_codes + 1


def tracked_quantities(vx, vy, tvx, tvy):
    """e2, s_e, dot, m as fp32 scalars, each product and sum rounded on its own"""
    with np.errstate(all="ignore"):
        vx, vy, tvx, tvy = F(vx), F(vy), F(tvx), F(tvy)
        ex, ey = F(vx - tvx), F(vy - tvy)
        e2 = F(F(ex * ex) + F(ey * ey))
        s_e = F(F(vx * vx) + F(vy * vy))
        s_t = F(F(tvx * tvx) + F(tvy * tvy))
        dot = F(F(vx * tvx) + F(vy * tvy))
        m = F(s_e * s_t)
    return e2, s_e, dot, m


def speed_bin(e2):
    return sum(1 for t in THRESHOLDS if e2 > F(t * t))


def direction_bin(s_e, dot, m):
    with np.errstate(all="ignore"):
        d2 = F(dot * dot)
        if s_e == F(0):
            return 4
        if dot > F(0) and d2 >= F(COS2_15 * m):
            return 0
        if dot > F(0) and d2 >= F(F(0.5) * m):
            return 1
    return 2 if dot > F(0) else 3


def e2_um(e2):
    with np.errstate(all="ignore"):
        clamped = e2 if e2 < F(1.0e4) else F(1.0e4)
        return int(F(clamped * F(1.0e6)))          # int() truncates toward zero


def audit_agent(born, src, n_in, truth_labels, codes, prm, ok=True, range_len=None, max_points=None):
    """born [n_born, 7] fp32, src [n_born] int, truth_labels [>= n_in, 4] fp32 and codes [>= n_in] int (or None) of THIS agent's
    input points, prm = dict(speed_tolerance, n_codes).  ok False, or n_in <= 0: SKIPPED.  range_len > max_points: CLIPPED
    (n_in is then max_points).  Returns (row [32] int64, table [n_codes + 2, 6] int64 or None)."""
    n_codes = int(prm["n_codes"])
    tol = F(prm["speed_tolerance"])
    row = np.zeros(ROW, np.int64)
    table = np.zeros((n_codes + 2, 6), np.int64) if codes is not None else None
    if range_len is not None and max_points is not None:
        n_in = min(int(range_len), int(max_points))
    if not ok or n_in <= 0:
        row[2] = SKIPPED
        return row, table
    if range_len is not None and max_points is not None and range_len > max_points:
        row[2] |= CLIPPED
    born = np.asarray(born, np.float32).reshape(-1, 7)
    row[0], row[1] = n_in, len(born)
    named = np.zeros(n_in, bool)

    def count(truth, est, i):
        row[4 + 4 * truth + est] += 1
        if table is not None:
            table[code_row(codes[i], n_codes), est] += 1

    for k in range(len(born)):
        i = int(src[k])
        if i < 0 or i >= n_in or named[i]:
            row[2] |= BAD_SOURCE
            continue
        named[i] = True
        vx, vy, _, inten = born[k, 3:7]
        tl = truth_labels[i]
        truth = truth_class(tl[3])
        est = estimate_class(vx, inten)
        count(truth, est, i)
        if est != TRACKED:
            continue
        tvx, tvy = (tl[0], tl[1]) if truth == MOVING else (F(0), F(0))
        e2, s_e, dot, m = tracked_quantities(vx, vy, tvx, tvy)
        if np.isnan(e2) or np.isnan(m):
            row[3] += 1
            continue
        within = int(e2 <= F(tol * tol))
        um = e2_um(e2)
        if table is not None:
            table[code_row(codes[i], n_codes), 4] += within
            table[code_row(codes[i], n_codes), 5] += um
        if truth == MOVING:
            row[12 + speed_bin(e2)] += 1
            row[24 + direction_bin(s_e, dot, m)] += 1
            row[29] += um
            row[30] += within
        else:
            row[18 + speed_bin(e2)] += 1
    for i in np.flatnonzero(~named):
        count(truth_class(truth_labels[i][3]), DROPPED, int(i))
    return row, table
