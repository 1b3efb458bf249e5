"""Independent numpy restatement (fp64) of the flight audit of include/sogm_abi.h ("flight audit"): record selection, the
100 Hz samples, the box and cylinder tests, the fold and the event order.  Every decision also yields its margin (distance
to its threshold), so that a comparison with the device can leave out the decisions that rounding could flip.
Not collected by pytest (helper module)."""
import math

import numpy as np

REC_BYTES = 2064
BODY = (0.4, 0.4, 0.45)
_A = np.array([[1, -4, 6, -4, 1], [0, 4, -12, 12, -4], [0, 0, 6, -12, 6], [0, 0, 0, 4, -4], [0, 0, 0, 0, 1]], np.float64)


def parse(rec):
    """one SogmTrajRecord (2064 bytes) -> (n_pieces, time_start, durations, cpts [16*5, 3])"""
    b = np.ascontiguousarray(rec, np.uint8)
    n = int(b[4:8].view(np.int32)[0])
    return n, float(b[8:16].view(np.float64)[0]), b[16:144].view(np.float64), b[144:].view(np.float64).reshape(-1, 3)


def record(time_start, durations, cpts, drone_id=0):
    """build a record: durations [n], cpts [n * 5, 3]"""
    b = np.zeros(REC_BYTES, np.uint8)
    n = len(durations)
    b[0:8] = np.array([drone_id, n], np.int32).view(np.uint8)
    b[8:16] = np.array([time_start], np.float64).view(np.uint8)
    d = np.zeros(16)
    d[:n] = durations
    b[16:144] = d.view(np.uint8)
    c = np.zeros((80, 3))
    c[:5 * n] = np.asarray(cpts, np.float64).reshape(-1, 3)
    b[144:] = c.reshape(-1).view(np.uint8)
    return b


def line_record(time_start, p0, v, duration):
    """one piece flying p0 + v (t - time_start) for `duration` seconds (then held)"""
    p0, v = np.asarray(p0, np.float64), np.asarray(v, np.float64)
    return record(time_start, [duration], [p0 + v * duration * (j / 4.0) for j in range(5)])


def eval_pos(rec, t):
    """position of a record at the times t (array), the Bezier evaluation clamped to the record's span"""
    n, ts, dur, cp = parse(rec)
    t = np.atleast_1d(np.asarray(t, np.float64))
    total = 0.0
    for k in range(n):
        total += dur[k]
    tt = np.clip(t - ts, 0.0, total)
    out = np.zeros((len(t), 3))
    for i, x in enumerate(tt):
        piece, rem = n - 1, x
        for k in range(n):
            rem -= dur[k]
            if rem < 0:
                piece = k
                break
        t0 = 0.0
        for k in range(piece):
            t0 += dur[k]
        d = (t0 + dur[piece]) - t0
        s = (x - t0) / d
        S0 = (1.0, s, s * s, s * s * s, (s * s) * (s * s))
        c = cp[piece * 5:piece * 5 + 5]
        for ax in range(3):
            p = 0.0
            for j in range(5):
                b = 0.0
                for q in range(5):
                    b += c[q, ax] * _A[q, j]
                p += b * S0[j]
            out[i, ax] = p
    return out


def new_acc(n):
    return {"min_gap": np.full(n, np.inf), "min_gap_time": np.full(n, -1.0), "min_sep": np.full(n, np.inf),
            "min_sep_time": np.full(n, -1.0), "goal_time": np.full(n, -1.0), "first_collision_time": np.full(n, -1.0),
            "path_length": np.zeros(n), "last_pos": np.zeros((n, 3)), "min_gap_obstacle": np.full(n, -1, np.int64),
            "min_sep_agent": np.full(n, -1, np.int64), "obstacle_samples": np.zeros(n, np.int64),
            "agent_samples": np.zeros(n, np.int64), "n_samples": np.zeros(n, np.int64), "has_last": np.zeros(n, np.int64)}


def cylinders(rows, z=2.0, h=4.0):
    """(n, 5) rows {x, y, w, vx, vy} (scene / WorldTimeline layout) -> (n, 7) {x, y, z, w, h, vx, vy}"""
    r = np.asarray(rows, np.float64).reshape(-1, 5)
    return np.stack([r[:, 0], r[:, 1], np.full(len(r), z), r[:, 2], np.full(len(r), h), r[:, 3], r[:, 4]], axis=1)


def sample_times(t0, first_tick, n_ticks, period, sample_dt):
    ratio = period / sample_dt
    m = int(round(ratio))
    if abs(ratio - m) > 1e-9 or m < 1:
        raise ValueError("period / sample_dt is not a whole number")
    return m, [(t0 + float(first_tick + k) * period) + float(j) * sample_dt for k in range(n_ticks) for j in range(m)]


def positions(tables, prev_table, fallback, t0, first_tick, period, sample_dt):
    """[samples][n_total][3] (the record selection compares times both sides build with the same expression: no margin)"""
    tables = np.asarray(tables, np.uint8)
    n_ticks, n_total = tables.shape[:2]
    m, ts = sample_times(t0, first_tick, n_ticks, period, sample_dt)
    pos = np.zeros((len(ts), n_total, 3))
    for k in range(n_ticks):
        tk = np.array(ts[k * m:(k + 1) * m])
        for a in range(n_total):
            cands = [tables[k, a]]
            if k > 0:
                cands.append(tables[k - 1, a])
            elif prev_table is not None:
                cands.append(np.asarray(prev_table, np.uint8)[a])
            got = np.zeros(m, bool)
            p = np.tile(np.asarray(fallback, np.float64)[a], (m, 1))
            for rec in cands:
                n, start, _, _ = parse(rec)
                if n <= 0:
                    continue
                use = ~got & (start <= tk)
                if use.any():
                    p[use] = eval_pos(rec, tk[use])
                got |= use
            pos[k * m:(k + 1) * m, a] = p
    return pos, ts


def audit(tables, prev_table, fallback, goals, cyl, t0, first_tick, period, agent0, n_local, t_obstacles=0.0,
          body=BODY, sample_dt=0.01, goal_tolerance=1.0, acc=None):
    """One call of the audit.  cyl: (n, 7) {x, y, z, w, h, vx, vy}.  Returns (acc, events [(t, agent, other, kind)],
    margins: list of arrays of |value - threshold| of every threshold decision taken; the minima are compared by value, ties between
    equal values go to the earliest sample and the lowest index)."""
    bx, by, bz = body
    margins = []
    pos, ts = positions(tables, prev_table, fallback, t0, first_tick, period, sample_dt)
    n_total = pos.shape[1]
    cyl = np.asarray(cyl, np.float64).reshape(-1, 7)
    goals = np.asarray(goals, np.float64).reshape(-1, 3)
    acc = new_acc(n_local) if acc is None else {k: v.copy() for k, v in acc.items()}
    events = []
    idx = np.arange(n_total)
    for s, t in enumerate(ts):
        P = pos[s]
        dtt = t - t_obstacles
        cx, cy = cyl[:, 0] + cyl[:, 5] * dtt, cyl[:, 1] + cyl[:, 6] * dtt
        for i in range(n_local):
            me = agent0 + i
            p = P[me]
            # agents
            d = p[None, :] - P
            sep = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            other = idx != me
            hit = other & (np.abs(d[:, 0]) < bx) & (np.abs(d[:, 1]) < by) & (np.abs(d[:, 2]) < bz)
            mb = np.minimum(np.minimum(np.abs(np.abs(d[:, 0]) - bx), np.abs(np.abs(d[:, 1]) - by)),
                            np.abs(np.abs(d[:, 2]) - bz))
            margins.append(mb[other])
            s_min, s_idx = np.inf, -1
            if other.any():
                so = np.where(other, sep, np.inf)
                s_idx = int(np.argmin(so))       # first of equal minima: the lowest index
                s_min = float(so[s_idx])
            # obstacles
            zdist = np.abs(p[2] - cyl[:, 2]) if len(cyl) else np.zeros(0)
            zlim = (cyl[:, 4] + bz) * 0.5 if len(cyl) else np.zeros(0)
            zov = zdist < zlim
            margins.append(np.abs(zdist - zlim))
            ex = np.maximum(np.abs(cx - p[0]) - bx * 0.5, 0.0)
            ey = np.maximum(np.abs(cy - p[1]) - by * 0.5, 0.0)
            gap = np.sqrt(ex * ex + ey * ey) - cyl[:, 3] * 0.5 if len(cyl) else np.zeros(0)
            ohit = zov & (gap < 0.0)
            margins.append(np.abs(gap[zov]))
            g_min, g_idx = np.inf, -1
            if zov.any():
                go = np.where(zov, gap, np.inf)
                g_idx = int(np.argmin(go))
                g_min = float(go[g_idx])
            for j in np.nonzero(hit)[0]:
                events.append((t, me, int(j), 0))
            for c in np.nonzero(ohit)[0]:
                events.append((t, me, int(c), 1))
            # fold
            if s_min < acc["min_sep"][i]:
                acc["min_sep"][i], acc["min_sep_time"][i], acc["min_sep_agent"][i] = s_min, t, s_idx
            if g_min < acc["min_gap"][i]:
                acc["min_gap"][i], acc["min_gap_time"][i], acc["min_gap_obstacle"][i] = g_min, t, g_idx
            acc["agent_samples"][i] += int(hit.any())
            acc["obstacle_samples"][i] += int(ohit.any())
            if (hit.any() or ohit.any()) and acc["first_collision_time"][i] < 0:
                acc["first_collision_time"][i] = t
            g = p - goals[i]
            dg = math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            if acc["goal_time"][i] < 0:
                margins.append(np.array([abs(dg - goal_tolerance)]))
                if dg < goal_tolerance:
                    acc["goal_time"][i] = t
            if acc["has_last"][i]:
                q = p - acc["last_pos"][i]
                acc["path_length"][i] += math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
            acc["last_pos"][i] = p
            acc["has_last"][i] = 1
    acc["n_samples"] += len(ts)
    return acc, events, margins


def near_threshold(margins, eps=1e-9):
    """number of decisions within eps of their threshold"""
    return int(sum(int((m < eps).sum()) for m in margins))


def _hover(n):
    return np.zeros((n, REC_BYTES), np.uint8)


def closed_form_cases():
    """Inputs of the closed-form cases and what they must give (analytic).  Each case: dict(name, tables [n_ticks][n][2064],
    prev_table, fallback [n][3], goals [n][3], cyl (k, 7), t0, first_tick, period, t_obstacles, expect)."""
    cases = []
    # head-on: two agents closing at 2 m/s along x; boxes touch while |dx| < 0.4, i.e. t in (0.805, 1.205): the sample
    # times sit half a sample from both contact instants -> samples 0.81 .. 1.20 (40); min centre distance 0.01
    D = 2.01
    recs = np.stack([line_record(0.0, (-D / 2, 0, 1), (1, 0, 0), 3.0), line_record(0.0, (D / 2, 0, 1), (-1, 0, 0), 3.0)])
    cases.append(dict(name="head_on", tables=np.stack([recs] * 20), prev_table=None, fallback=np.zeros((2, 3)),
                      goals=np.array([[10.0, 0, 1], [-10.0, 0, 1]]), cyl=np.zeros((0, 7)), t0=0.0, first_tick=0,
                      period=0.1, t_obstacles=0.0,
                      expect=dict(agent_samples=[40, 40], min_sep=[0.01, 0.01], first_collision_time=[0.81, 0.81],
                                  n_events=80)))
    # a straight pass at 1 m/s beside a static cylinder (w 0.5) at lateral offset d: min gap d - 0.2 - w / 2, reached
    # while the axis is within the body's half width of x (|x - 5| <= 0.2: t in [4.8, 5.2]); at d = 0.3 the gap is below
    # zero while |x - 5| < sqrt(0.25^2 - 0.1^2) + 0.2 = 0.429129: samples 4.58 .. 5.42 (85)
    for d, n_coll in ((1.0, 0), (0.3, 85)):
        cases.append(dict(name=f"static_cylinder_{d}", tables=np.stack([line_record(0.0, (0, 0, 1), (1, 0, 0), 10.0)[None]] * 60),
                          prev_table=None, fallback=np.zeros((1, 3)), goals=np.array([[20.0, 0, 1]]),
                          cyl=np.array([[5.0, d, 2.0, 0.5, 4.0, 0.0, 0.0]]), t0=0.0, first_tick=0, period=0.1,
                          t_obstacles=0.0,
                          expect=dict(obstacle_samples=[n_coll], min_gap=[d - 0.2 - 0.25], min_gap_time_in=(4.8, 5.2),
                                      n_events=n_coll)))
    # a cylinder (w 0.6) sweeping at 1 m/s through a hovering agent: axis x = -3.005 + t, collision while |x| < 0.5:
    # t in (2.505, 3.505) -> samples 2.51 .. 3.50 (100)
    cases.append(dict(name="moving_cylinder", tables=np.stack([_hover(1)] * 50), prev_table=None,
                      fallback=np.array([[0.0, 0, 1]]), goals=np.array([[9.0, 0, 1]]),
                      cyl=np.array([[-3.005, 0.0, 2.0, 0.6, 4.0, 1.0, 0.0]]), t0=0.0, first_tick=0, period=0.1,
                      t_obstacles=0.0,
                      expect=dict(obstacle_samples=[100], first_collision_time=[2.51], min_gap=[-0.3], n_events=100)))
    # goal: x = 0.005 + t towards (5, 0, 1): inside 1.0 m once t > 3.995 -> the sample 4.00
    cases.append(dict(name="goal", tables=np.stack([line_record(0.0, (0.005, 0, 1), (1, 0, 0), 6.0)[None]] * 50),
                      prev_table=None, fallback=np.zeros((1, 3)), goals=np.array([[5.0, 0, 1]]), cyl=np.zeros((0, 7)),
                      t0=0.0, first_tick=0, period=0.1, t_obstacles=0.0,
                      expect=dict(goal_time=[4.0], path_length=[4.99])))
    # record switch at tick 1 (t_1 = 0.1): agent 1's old record sits on agent 0; its new one starts at t_1 + 0.02 far away:
    # exactly the samples t_1 and t_1 + 0.01 collide
    t1 = 0.0 + 1.0 * 0.1
    old = np.stack([line_record(0.0, (0, 0, 1), (0, 0, 0), 5.0), line_record(0.0, (0.1, 0, 1), (0, 0, 0), 5.0)])
    new = old.copy()
    new[1] = line_record(t1 + 2.0 * 0.01, (5.0, 0, 1), (0, 0, 0), 5.0)
    cases.append(dict(name="record_switch", tables=new[None], prev_table=old, fallback=np.zeros((2, 3)),
                      goals=np.array([[9.0, 0, 1], [9.0, 0, 1]]), cyl=np.zeros((0, 7)), t0=0.0, first_tick=1,
                      period=0.1, t_obstacles=0.0,
                      expect=dict(agent_samples=[2, 2], first_collision_time=[0.1, 0.1], n_events=4,
                                  event_times=[0.1, 0.1, 0.11, 0.11])))
    # fallback: no record at all, the agent hovers at its start
    cases.append(dict(name="fallback", tables=np.stack([_hover(1)] * 5), prev_table=None,
                      fallback=np.array([[1.0, 2.0, 1.5]]), goals=np.array([[1.5, 2.0, 1.5]]), cyl=np.zeros((0, 7)),
                      t0=3.0, first_tick=0, period=0.1, t_obstacles=3.0,
                      expect=dict(goal_time=[3.0], path_length=[0.0], last_pos=[[1.0, 2.0, 1.5]], n_samples=[50])))
    return cases


def run_case(c, acc=None):
    return audit(c["tables"], c["prev_table"], c["fallback"], c["goals"], c["cyl"], c["t0"], c["first_tick"], c["period"],
                 0, c["tables"].shape[1], t_obstacles=c["t_obstacles"], acc=acc)


def check_expect(c, acc, events):
    """assert the analytic values of a case (distances and times to 1e-9)"""
    for k, want in c["expect"].items():
        if k == "n_events":
            assert len(events) == want, (c["name"], len(events), want)
        elif k == "event_times":
            np.testing.assert_allclose([e[0] for e in events], want, atol=1e-12, err_msg=c["name"])
        elif k == "min_gap_time_in":
            lo, hi = want
            assert np.all((acc["min_gap_time"] >= lo - 1e-9) & (acc["min_gap_time"] <= hi + 1e-9)), (c["name"], acc["min_gap_time"])
        elif acc[k].dtype.kind == "i":
            assert np.array_equal(acc[k], np.asarray(want)), (c["name"], k, acc[k], want)
        else:
            np.testing.assert_allclose(acc[k], want, atol=1e-9, err_msg=f"{c['name']} {k}")
