"""Inputs shared by tests/test_velocity_audit_host.py and tests/test_velocity_audit_gpu.py: the seeded truth arrays over
helpers.velocity_fixture_inputs(), and the hand-built rows that sit on every comparison of the rule."""
import numpy as np

N_CODES = 7
TOLERANCE = 0.25
SEED = 0x7E1A
f32 = np.float32
# truth velocities (label_of's shape: {vx, vy, vz, 1} or zeros).  The fixture's clusters step 0.25 m per 0.5 s along an axis:
# against an estimate of (0.5, 0) these give speed-error bins 0 .. 5 ((0.5, 0): 0; (0.65, 0): 0.15; (0.5, 0.4): 0.4; (0.1, 0.6):
# 0.72; (-1, 0): 1.5; (3, 0): 2.5) and directions within 15, within 45, ahead, and behind.
MENU = f32([[0.5, 0.0], [0.0, 0.5], [-0.5, 0.0], [0.0, -0.5], [0.65, 0.0], [0.5, 0.4], [0.1, 0.6], [-1.0, 0.0], [3.0, 0.0]])


def truth_arrays(index, n):
    """(labels [n, 4] fp32, codes [n] int32) of sequence `index`'s last cloud: codes in [-2, N_CODES + 1], about half the
    points moving with a velocity from MENU and vz in {0, 0.25}, and a few NaN rows (a NaN velocity on a moving point, a NaN
    intensity)"""
    rng = np.random.default_rng([SEED, index])
    codes = rng.integers(-2, N_CODES + 2, size=n).astype(np.int32)
    labels = np.zeros((n, 4), f32)
    moving = rng.random(n) < 0.5
    pick = rng.integers(0, len(MENU), size=n)
    labels[moving, :2] = MENU[pick[moving]]
    labels[moving, 2] = f32(0.25) * (rng.random(n)[moving] < 0.3)
    labels[moving, 3] = f32(1.0)
    odd = rng.random(n) < 0.02
    kind = rng.integers(0, 3, size=n)
    labels[odd & (kind == 0), 0] = np.nan                      # vx NaN: a moving point's e2 is NaN, a still point's is not read
    labels[odd & (kind == 1), 1] = np.nan
    labels[odd & (kind == 2), 3] = np.nan                      # intensity NaN: STILL
    return labels, codes


def h32(v):
    return " ".join("%08x" % int(x) for x in np.ascontiguousarray(v, f32).reshape(-1).view(np.uint32))


def case_line(born, src, truth, codes, tol, n_codes, ok=True, range_len=None, max_points=64):
    """one line of tests/velaudit_rules_host_test.cpp's input"""
    born = np.asarray(born, f32).reshape(-1, 7)
    truth = np.asarray(truth, f32).reshape(-1, 4)
    range_len = len(truth) if range_len is None else range_len
    parts = ["A", str(int(ok)), str(range_len), str(max_points), str(n_codes), "0" if codes is None else "1", h32([tol]), str(len(born))]
    for r, s in zip(born, src):
        parts += [h32(r), str(int(s))]
    parts.append(str(len(truth)))
    for i, t in enumerate(truth):
        parts += [h32(t), str(0 if codes is None else int(codes[i]))]
    return " ".join(parts)


def _row(vx, vy, inten, vz=0.0):
    return [1.0, 2.0, 0.5, vx, vy, vz, inten]


def hand_built():
    """name -> dict(born, src, truth, codes, tol, n_codes, ok, range_len, max_points): rows on every comparison of the rule"""
    inf, nan = np.inf, np.nan
    I001, below, above = f32(0.01), np.nextafter(f32(0.01), f32(0)), np.nextafter(f32(0.01), f32(1))
    out = {}

    def case(name, rows, truth, codes=None, src=None, tol=TOLERANCE, n_codes=3, **kw):
        rows = np.asarray(rows, f32).reshape(-1, 7)
        truth = np.asarray(truth, f32).reshape(-1, 4)
        out[name] = dict(born=rows, src=np.arange(len(rows)) if src is None else np.asarray(src), truth=truth,
                         codes=None if codes is None else np.asarray(codes, np.int64), tol=tol, n_codes=n_codes, **kw)

    # intensity exactly 0.01f is not above it (STATIC / STILL), one float above is; vx exactly -100 is UNTRACKED
    est = [_row(0.5, 0, I001), _row(0.5, 0, above), _row(0.5, 0, below), _row(-100.0, 0, 1), _row(np.nextafter(f32(-100), f32(0)), 0, 1),
           _row(-10000.0, -10000.0, 0.55, -10000.0), _row(0.5, 0, nan), _row(nan, 0, 1)]
    tru = [[0.5, 0, 0, I001], [0.5, 0, 0, above], [0.5, 0, 0, below], [0, 0, 0, 0], [-100, 0, 0, 1], [1, 1, 0, 1], [0, 0, 0, nan], [0.5, 0, 0, 1]]
    case("intensity and vx ties", est, tru, codes=[0, 1, 2, 3, -1, -2, -3, np.iinfo(np.int32).min])
    # e2 == T*T for every T, and one float above: estimate (T, 0) or just above against a moving truth of (0, 1e-30) (s_t > 0 but
    # its products underflow: e2 is T*T exactly), and against a still truth
    rows, tru = [], []
    for T in (0.1, 0.25, 0.5, 1.0, 2.0):
        for v in (f32(T), np.nextafter(f32(T), f32(9)), -f32(T)):
            rows += [_row(v, 0, 1), _row(v, 0, 1), _row(0, v, 0.55)]
            tru += [[0, 0, 0, 1], [9, 9, 9, 0], [0, 0, 0, 1]]
    case("speed ties", rows, tru, codes=np.arange(len(rows)) % 5 - 2, n_codes=2)
    # tolerance: e2 == tol*tol is within, one float above is not; tol = 0 takes only an exact estimate
    rows = [_row(1.25, 0.5, 1), _row(np.nextafter(f32(1.25), f32(9)), 0.5, 1), _row(1.0, 0.75, 1), _row(1.0, 0.5, 1)]
    tru = [[1.0, 0.5, 0, 1]] * 4
    case("tolerance tie", rows, tru, codes=[0, 0, 1, 1], tol=0.25)
    case("tolerance zero", rows, tru, codes=[0, 0, 1, 1], tol=0.0)
    # direction: dot*dot == 0.5f*m exactly at 45 degrees ((1, 0) against (1, 1): dot 1, m 2); a hair inside 15 degrees and outside;
    # dot == 0; dot < 0; s_e == 0 with a moving truth; s_t == 0 is not possible for a MOVING label unless its velocity is zero
    c15, s15 = np.cos(np.radians(14.9)), np.sin(np.radians(14.9))
    c16, s16 = np.cos(np.radians(15.1)), np.sin(np.radians(15.1))
    rows = [_row(1, 0, 1), _row(1, 0, 1), _row(1, 0, 1), _row(1, 0, 1), _row(1, 0, 1), _row(1, 0, 1), _row(0, 0, 1), _row(0.0, -0.0, 1),
            _row(1, 0, 1), _row(2, 0, 1)]
    tru = [[1, 1, 0, 1], [1, np.nextafter(f32(1), f32(9)), 0, 1], [c15, s15, 0, 1], [c16, s16, 0, 1], [0, 1, 0, 1], [-1, 0.5, 0, 1],
           [0.5, 0, 0, 1], [0, 0, 0, 1], [0, 0, 7, 1], [1, 0, 0, 1]]
    case("direction ties", rows, tru, codes=[5, 4, 3, 2, 1, 0, -1, -2, 3, 3], n_codes=4)
    # NaN and +-inf in either label; e2 above the clamp (101 m/s of error: e2 = 10201) and far above it (1e30: e2 = +inf)
    rows = [_row(inf, 0, 1), _row(-inf, 0, 1) , _row(inf, 0, 1), _row(0.5, inf, 1), _row(0.5, 0, inf), _row(0.5, 0, -inf), _row(nan, nan, 1),
            _row(0.5, nan, 1), _row(101.0, 0, 1), _row(1e30, 0, 1), _row(1e30, 0, 1), _row(0.5, 0, 1), _row(0.5, 0, 1), _row(0.5, 0, 1),
            _row(0.5, 0, 1), _row(60.0, 80.0, 1)]
    tru = [[1, 0, 0, 1], [0, 0, 0, 0], [inf, 0, 0, 1], [0, 1, 0, 1], [0.5, 0, 0, 1], [0.5, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 1],
           [0, 1e-30, 0, 1], [0, 0, 0, 0], [-1e30, 0, 0, 1], [inf, 0, 0, 1], [0, -inf, 0, inf], [nan, 0, 0, 1], [nan, nan, nan, 0],
           [0, 1e-30, 0, 1]]
    case("nan inf clamp", rows, tru, codes=[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0])
    # codes -1 (ground), -2 (none), n_codes and INT32_MIN with every estimate class, one dropped point per code
    codes = [-1, -2, 3, np.iinfo(np.int32).min, 0, 2, np.iinfo(np.int32).max] * 2
    rows = [_row(0.5, 0, 1), _row(0, 0, 0), _row(-10000, -10000, 0.55), _row(0.5, 0.1, 1), _row(0, 0, 0), _row(0.4, 0, 1), _row(0.5, 0, 1)]
    tru = [[0.5, 0, 0, 1], [0, 0, 0, 0]] * 7
    case("codes", rows, tru, codes=codes, src=[0, 1, 2, 3, 4, 5, 6])
    # a duplicated source (the second row that names point 1 is ignored, whatever it says) and sources out of range
    rows = [_row(0.5, 0, 1), _row(0.5, 0, 1), _row(-10000, 0, 1), _row(0, 0, 0), _row(0.5, 0, 1), _row(0.5, 0, 1), _row(0.25, 0, 1)]
    tru = [[0.5, 0, 0, 1], [0.5, 0, 0, 1], [0, 0, 0, 0], [0.5, 0, 0, 1], [0, 0, 0, 0]]
    case("bad sources", rows, tru, codes=[0, 1, 2, -1, 0], src=[1, 0, 1, -1, 5, np.iinfo(np.int32).max, 3])
    case("no codes", rows[:2], tru[:3], codes=None, src=[2, 0])
    case("n_born zero", np.zeros((0, 7)), tru, codes=[0, 1, 2, -1, -2])
    case("n_in zero", np.zeros((0, 7)), np.zeros((0, 4)), codes=[])
    case("rejected update", rows[:2], tru[:3], codes=[0, 0, 0], src=[0, 1], ok=False)
    case("clipped", rows[:4], tru[:4], codes=[0, 1, 2, 2], src=[3, 2, 1, 0], range_len=9, max_points=4)
    case("n_codes zero", rows[:4], tru[:4], codes=[0, -1, -2, 5], src=[3, 2, 1, 0], n_codes=0)
    return out
