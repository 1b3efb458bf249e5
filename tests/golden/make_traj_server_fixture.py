"""Writes tests/golden/traj_server_independent.json: a second reading of the reference's trajectory server in plain Python.

Written from traj_server/src/bezier_traj_server.cpp (bezierCallback :283-355, resetTrajQueue :233-244, mergeTrajQueue
:246-277, PubCallback :415-485, fillTrajQueue :211-228, getYaw :79-140, pushToTrajQueue as bezier_traj_server_rotors.cpp
:212-223 has it) and from the definition in include/sogm_abi.h "trajectory server" (the clamped evaluation, the ring's
bound of 256 samples, when a tick's record arrives) — NOT from csrc/sogm_trajserver.hpp.  A collections.deque is the
queue, the Bezier pieces are evaluated in the Bernstein basis (the product evaluates the monomial form), atan2 is a
restatement of sogm_det::atan2 (include/sogm_detmath.h) operation for operation.

Decisions that depend on times alone use the reference's IEEE expressions and must come out EQUAL in the product.  Decisions
that depend on evaluated values — getYaw's comparisons, dir.norm() > 0.1 — are counted when they lie within 1e-9 of their
threshold (near_threshold's convention in tests/swarm_audit_reference.py) and the fixture is refused unless that count is
0.  A comparison "depends on evaluated values" once an evaluated velocity has reached its operands: while last_yaw is still
an exact function of init_yaw and the constants (the saturated steps yaw = last_yaw -+ MAX_YAW_CHANGE before the first
tracked one) both readings hold the same bits, and |yaw - last_yaw| <= MAX_YAW_CHANGE — which sits on its threshold by
construction there — is not a decision between them; the cases turn first and track afterwards.

Run: python tests/golden/make_traj_server_fixture.py"""
import json
import math
import os
import random
from collections import deque

QUEUE = 256
EPS = 1e-9
LAUNCHED = (3.14159265358979323846, 3.14159265358979323846)   # bezier_traj_server.cpp:35-36
ROTORS = (3.1415926, 0.05)                                     # bezier_traj_server_rotors.cpp:36, :78


# ---- sogm_det::atan2, restated ----
AT_HI = [0.0, 0.12435499454676144, 0.24497866312686414, 0.35877067027057225, 0.4636476090008061, 0.5585993153435624,
         0.6435011087932844, 0.7188299996216245, 0.7853981633974483]
AT_LO = [0.0, -3.1253241424539383e-18, 1.0698755618734451e-17, -2.4623815582638635e-17, 2.2698777452961687e-17,
         -5.4556305485916264e-18, 1.5834785051444286e-17, -2.1478388444456983e-17, 3.061616997868383e-17]
PI_HI, PI_LO = 3.141592653589793, 1.2246467991473532e-16
PIO2_HI, PIO2_LO = 1.5707963267948966, 6.123233995736766e-17


def det_atan2(y, x):
    yneg, xneg = math.copysign(1.0, y) < 0, math.copysign(1.0, x) < 0
    ay, ax = abs(y), abs(x)
    if ay == 0.0:
        a = PI_HI if xneg else 0.0
    elif ax == 0.0:
        a = PIO2_HI
    else:
        steep = ay > ax
        t = ax / ay if steep else ay / ax
        k = int(t * 8.0 + 0.5)
        c = k * 0.125
        r = (t - c) / (1.0 + t * c)
        z = r * r
        p = 1.0 / 17.0
        for num, den in ((-1.0, 15.0), (1.0, 13.0), (-1.0, 11.0), (1.0, 9.0), (-1.0, 7.0), (1.0, 5.0), (-1.0, 3.0)):
            p = p * z + num / den
        a0 = AT_HI[k] + ((r + r * (z * p)) + AT_LO[k])
        if steep:
            a = PIO2_HI + (a0 + PIO2_LO) if x < 0 else PIO2_HI - (a0 - PIO2_LO)
        else:
            a = PI_HI - (a0 - PI_LO) if x < 0 else a0
    return -a if yneg else a


# ---- a trajectory: durations + control points, evaluated in the Bernstein basis, t clamped to [0, total] ----
def bernstein(n, i, s):
    return math.comb(n, i) * s ** i * (1.0 - s) ** (n - i)


def evaluate(rec, t):
    dur, cp = rec["duration"], rec["cpts"]
    total = 0.0
    for d in dur:
        total += d
    t = 0.0 if t < 0 else (total if t > total else t)
    piece, rem = len(dur) - 1, t
    for i, d in enumerate(dur):   # locatePiece (bernstein.hpp:164-172)
        rem -= d
        if rem < 0:
            piece = i
            break
    t0 = 0.0
    for d in dur[:piece]:
        t0 += d
    T = (t0 + dur[piece]) - t0
    s = (t - t0) / T
    c = cp[piece * 5:piece * 5 + 5]
    pos = [sum(bernstein(4, i, s) * c[i][d] for i in range(5)) for d in range(3)]
    vel = [4.0 / T * sum(bernstein(3, i, s) * (c[i + 1][d] - c[i][d]) for i in range(4)) for d in range(3)]
    acc = [12.0 / (T * T) * sum(bernstein(2, i, s) * (c[i + 2][d] - 2.0 * c[i + 1][d] + c[i][d]) for i in range(3))
           for d in range(3)]
    return pos, vel, acc


class Server:
    def __init__(self, prm, t_trigger, init_pos, init_yaw):
        self.thres, self.dt, self.pi, self.rate, self.mode = (prm["replan_threshold"], prm["sample_dt"], prm["yaw_pi"],
                                                              prm["yaw_dot_max"], prm["yaw_mode"])
        self.q = deque()
        self.ti = self.ts = self.te = t_trigger
        self.duration = 0.0
        self.last_yaw, self.last_yawdot = init_yaw, 0.0
        self.init_pos = list(init_pos)
        self.traj, self.traj_id, self.received, self.overflow = None, 0, False, False
        self.tainted = False      # an evaluated velocity has reached last_yaw
        self.near = 0             # value-dependent decisions within EPS of their threshold
        self.leaves = set()
        self.min_vxy = math.inf

    # a comparison of getYaw: lhs `op` rhs; counted when evaluated values reach it and it is within EPS of flipping
    def _cmp(self, lhs, op, rhs, depends):
        if depends and abs(lhs - rhs) < EPS:
            self.near += 1
        return {">": lhs > rhs, "<": lhs < rhs, "<=": lhs <= rhs}[op]

    def get_yaw(self, v):
        PI, RATE, MAXC = self.pi, self.rate, self.rate * 0.01
        last = self.last_yaw
        z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        d = [x / math.sqrt(z) for x in v] if z > 0 else list(v)   # Eigen's normalized()
        norm = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        moving = self._cmp(norm, ">", 0.1, True)
        if moving:
            self.min_vxy = min(self.min_vxy, math.hypot(v[0], v[1]))
        yaw_temp = det_atan2(d[1], d[0]) if moving else last
        dep = self.tainted or moving
        diff = yaw_temp - last
        if self._cmp(diff, ">", PI, dep):
            if self._cmp(yaw_temp - last - 2 * PI, "<", -MAXC, dep):
                yaw = last - MAXC
                if self._cmp(yaw, "<", -PI, self.tainted):
                    yaw += 2 * PI
                    self.leaves.add("A.turn.wrap")
                yaw_dot = -RATE
                track = False
                self.leaves.add("A.turn")
            else:
                yaw, yaw_dot, track = yaw_temp, -RATE, True   # (yaw - last > PI is the branch's own condition)
                self.leaves.add("A.take")
        elif self._cmp(diff, "<", -PI, dep):
            if self._cmp(yaw_temp - last + 2 * PI, ">", MAXC, dep):
                yaw = last + MAXC
                if self._cmp(yaw, ">", PI, self.tainted):
                    yaw -= 2 * PI
                    self.leaves.add("B.turn.wrap")
                yaw_dot = RATE
                track = False
                self.leaves.add("B.turn")
            else:
                yaw, yaw_dot, track = yaw_temp, RATE, True
                self.leaves.add("B.take")
        else:
            if self._cmp(diff, "<", -MAXC, dep):
                yaw = last - MAXC
                if self._cmp(yaw, "<", -PI, self.tainted):
                    yaw += 2 * PI
                    self.leaves.add("C.down.wrap")
                yaw_dot, track = -RATE, False
                self.leaves.add("C.down")
            elif self._cmp(diff, ">", MAXC, dep):
                yaw = last + MAXC
                if self._cmp(yaw, ">", PI, self.tainted):
                    yaw -= 2 * PI
                    self.leaves.add("C.up.wrap")
                yaw_dot, track = RATE, False
                self.leaves.add("C.up")
            else:
                yaw, track = yaw_temp, moving
                yaw_dot = (yaw_temp - last) / 0.01   # (|diff| <= MAX_YAW_CHANGE: neither of the two PI tests can hold)
                self.leaves.add("C.track" if moving else "C.hold")
        if track:
            self.tainted = True
        if self._cmp(abs(yaw - last), "<=", MAXC, self.tainted):
            yaw = 0.5 * last + 0.5 * yaw
        yaw_dot = 0.5 * self.last_yawdot + 0.5 * yaw_dot
        self.last_yaw, self.last_yawdot = yaw, yaw_dot
        return yaw, yaw_dot

    def push(self, t, traj):     # pushToTrajQueue on the bounded ring
        if len(self.q) >= QUEUE:
            self.overflow = True
            return
        pos, vel, acc = evaluate(traj, t)
        yaw, yaw_dot = self.get_yaw(vel) if self.mode == 1 else (0.0, 0.0)
        self.q.append({"t": self.ts + t, "pos": pos, "vel": vel, "acc": acc, "yaw": yaw, "yaw_dot": yaw_dot})

    def bezier_callback(self, rec, now):
        tns = rec["time_start"]
        duration = 0.0
        for d in rec["duration"]:
            duration += d
        if self.te <= tns:
            branch = "reset"
            self.q.clear()
            t = 0.0
            while t < self.thres:
                self.push(t, rec)
                t += self.dt
        else:
            quot = (now + self.thres - tns) / self.dt
            k = int(quot) if -2147483648.0 < quot < 2147483648.0 else -1
            if k < 0 or k > len(self.q):
                branch = "early" if k >= 0 else "early(k<0)"
                dt = now - tns
                i = 0
                while i < self.thres / self.dt:
                    self.push(i * self.dt + dt, rec)
                    i += 1
            else:
                branch = "merge"
                for _ in range(k):
                    self.q.pop()
                for i in range(k):
                    self.push(i * self.dt, rec)
            branch += f" k={k}"
        self.traj = rec
        self.duration = duration
        self.ts = tns
        self.te = self.ts + self.duration
        self.traj_id += 1
        self.received = True
        return branch

    def pub_callback(self, now):
        none = {"t_pub": now, "t_sample": 0.0, "pos": list(self.init_pos), "vel": [0.0] * 3, "acc": [0.0] * 3, "yaw": 0.0,
                "yaw_dot": 0.0, "traj_id": 0, "flags": 0}
        if not self.received or not self.q:
            return none, "silent"
        if len(self.q) == 1:
            p = self.q[0]
            return {"t_pub": now, "t_sample": p["t"], "pos": p["pos"], "vel": [0.0] * 3, "acc": [0.0] * 3,
                    "yaw": self.last_yaw, "yaw_dot": 0.0, "traj_id": self.traj_id, "flags": 3}, "held"
        p = self.q.popleft()
        tq = now + self.thres
        what = "pop"
        if tq < self.ts:
            what = "pop,tq<ts"
        else:
            t = tq - self.ts
            if t > self.duration:
                what = "pop,t>duration"
            else:
                self.push(t, self.traj)
        return {"t_pub": now, "t_sample": p["t"], "pos": p["pos"], "vel": p["vel"], "acc": p["acc"], "yaw": p["yaw"],
                "yaw_dot": p["yaw_dot"], "traj_id": self.traj_id, "flags": 1}, what


def run_case(case):
    prm = case["prm"]
    s = Server(prm, case["t_trigger"], case["init_pos"], case["init_yaw"])
    m = int(round(case["period"] / prm["sample_dt"]))
    assert abs(case["period"] / prm["sample_dt"] - m) <= 1e-9
    cmds, sizes, branches = [], [], set()
    for k, tick in enumerate(case["ticks"]):
        t_k = case["t0"] + (case["first_tick"] + k) * case["period"]
        t_rcv = t_k + case["receive_delay"]
        j_rcv = 0
        while j_rcv < m and t_k + j_rcv * prm["sample_dt"] < t_rcv:
            j_rcv += 1
        for j in range(m + 1):
            if j == j_rcv and tick["received"] and tick["record"] is not None:
                b = s.bezier_callback(case["records"][tick["record"]], t_rcv)
                branches.add(b.split(" k=")[0])
                case.setdefault("branches", []).append(b)
                sizes.append(len(s.q))
            if j < m:
                c, what = s.pub_callback(t_k + j * prm["sample_dt"])
                branches.add(what)
                cmds.append([c["t_pub"], c["t_sample"]] + c["pos"] + c["vel"] + c["acc"] + [c["yaw"], c["yaw_dot"],
                                                                                             c["traj_id"], c["flags"]])
                sizes.append(len(s.q))
    case["m"] = m
    case["commands"] = cmds
    case["sizes"] = sizes      # queue size after every event (arrivals and timers, in order)
    case["final"] = {"ts": s.ts, "te": s.te, "duration": s.duration, "last_yaw": s.last_yaw, "last_yawdot": s.last_yawdot,
                     "size": len(s.q), "traj_id": s.traj_id, "received": int(s.received), "overflow": int(s.overflow)}
    case["queue"] = [[p["t"], p["yaw"], p["yaw_dot"]] for p in s.q]
    return s, branches


# ---- the cases ----
def line_record(start, p0, heading, speed, n_pieces=1, piece=0.8, vz=0.0):
    """constant velocity along `heading` (radians): five evenly spaced control points per piece"""
    dur = [piece] * n_pieces
    cp, x = [], list(p0)
    step = [speed * piece / 4.0 * math.cos(heading), speed * piece / 4.0 * math.sin(heading), vz * piece / 4.0]
    for _ in range(n_pieces):
        for i in range(5):
            cp.append([x[0] + i * step[0], x[1] + i * step[1], x[2] + i * step[2]])
        x = cp[-1]
    return {"time_start": start, "duration": dur, "cpts": cp}


def curved_record(rng, start, n_pieces, piece, p0=(0.0, 0.0, 1.0), speed=1.5):
    """a smooth random curve: control points advance mostly along +x with small sideways steps (|v_xy| stays well above 1e-3
    and the heading turns far slower than MAX_YAW_CHANGE per sample); values rounded to 1e-3 to keep the file small"""
    dur = [piece] * n_pieces
    cp, x = [], list(p0)
    for _ in range(n_pieces):
        for i in range(5):
            if i:
                x = [round(x[0] + speed * piece / 4.0 * rng.uniform(0.9, 1.1), 3),
                     round(x[1] + speed * piece / 4.0 * rng.uniform(-0.005, 0.005), 3), round(x[2] + rng.uniform(-0.01, 0.01), 3)]
            cp.append(list(x))
    return {"time_start": start, "duration": dur, "cpts": cp}


def hover_record(start, p):
    return {"time_start": start, "duration": [0.5], "cpts": [list(p)] * 5}    # publishEmptyTrajectory's record


def params(thres, mode=0, const=LAUNCHED):
    return {"replan_threshold": thres, "sample_dt": 0.01, "yaw_pi": const[0], "yaw_dot_max": const[1], "yaw_mode": mode}


def make_case(name, prm, records, ticks, t0=10.0, first_tick=0, period=0.1, receive_delay=0.0, init_yaw=0.0,
              init_pos=(0.5, -0.25, 1.0), infer=False):
    """ticks: per tick None (nothing arrives) or a record index; infer: the product may be run with received = NULL"""
    return {"name": name, "prm": prm, "t_trigger": t0 - 3.0, "init_pos": list(init_pos), "init_yaw": init_yaw, "t0": t0,
            "first_tick": first_tick, "period": period, "receive_delay": receive_delay, "infer": infer, "records": records,
            "ticks": [{"record": r, "received": int(r is not None)} for r in ticks]}


def stamp(t0, k, period=0.1):
    return t0 + k * period


def build_cases():
    rng = random.Random(0x7a6a)
    cases = []
    t0 = 10.0
    # the reset on the first trajectory (te <= tns) and the skew: the record starts at stamp + 0.02 (replan_start_time) and its
    # first sample is flown at the stamp; then a merge, then a tick in which nothing arrives
    for rst, thres in ((0.02, 0.5), (0.1, 0.3)):
        recs = [curved_record(rng, stamp(t0, 0) + rst, 4, 0.8), curved_record(rng, stamp(t0, 1) + rst, 4, 0.8)]
        cases.append(make_case(f"reset_first_then_merge_rst{rst}_thres{thres}", params(thres), recs, [0, 1, None], infer=True))
    # merges at the launch files' thresholds; 1.2 with replan_start_time 0.02 has k = 118: two trips of 64 lanes
    # (the truncated IEEE quotient (now + 1.2 - tns) / 0.01 is 117 with stamps near 10 s and 118 with stamps near 100 s)
    for thres, tb in ((0.02, t0), (0.3, t0), (1.2, t0), (1.2, 100.0)):
        recs = [curved_record(rng, stamp(tb, 3), 4, 0.8), curved_record(rng, stamp(tb, 4) + 0.02, 4, 0.8),
                curved_record(rng, stamp(tb, 5) + 0.02, 4, 0.8)]
        cases.append(make_case(f"merge_thres{thres}_t{tb:g}", params(thres, 1), recs, [0, 1, 2], t0=tb, first_tick=3,
                               infer=True))
    # an arrival whose start lies before the buffer (k > size), received 35 ms into the tick
    recs = [curved_record(rng, stamp(t0, 0), 4, 0.8), curved_record(rng, stamp(t0, 1) - 0.5, 4, 0.8)]
    cases.append(make_case("early_start_before_buffer", params(0.3), recs, [0, 1], receive_delay=0.035, infer=True))
    # a negative k (the start is far ahead: the int is compared as a size_t), then tq < ts pops without pushing
    recs = [curved_record(rng, stamp(t0, 0), 4, 0.8), curved_record(rng, stamp(t0, 1) + 1.0, 4, 0.8)]
    cases.append(make_case("negative_k_then_tq_lt_ts", params(0.3, 1), recs, [0, 1, None], infer=True))
    # the first record starts beyond the look-ahead: tq < ts from the start
    cases.append(make_case("first_record_ahead_tq_lt_ts", params(0.3), [curved_record(rng, stamp(t0, 0) + 0.6, 2, 0.8)], [0]))
    # a trajectory that ends: the queue drains to one sample, which is held; then a reset after that end
    recs = [line_record(stamp(t0, 0), (0.0, 0.0, 1.0), 0.3, 1.0, 1, 0.4), line_record(stamp(t0, 6) + 0.02, (0.4, 0.1, 1.0), 0.31, 1.0, 2, 0.8)]
    cases.append(make_case("ends_drains_held_then_reset", params(0.3, 1), recs, [0, None, None, None, None, None, 1]))
    # no trajectory yet (records without pieces), then the first one
    cases.append(make_case("no_trajectory_yet", params(0.5), [curved_record(rng, stamp(t0, 2), 2, 0.8)], [None, None, 0]))
    # a 16-piece record
    recs = [curved_record(rng, stamp(t0, 0), 16, 0.25), curved_record(rng, stamp(t0, 1) + 0.02, 16, 0.25)]
    cases.append(make_case("sixteen_pieces", params(0.5, 1), recs, [0, 1]))
    # a one-piece hover record with zero velocity behind a moving one: yaw is held
    recs = [line_record(stamp(t0, 0), (1.0, 2.0, 1.0), 0.7, 1.2, 2, 0.8), hover_record(stamp(t0, 1) + 0.02, (1.5, 2.5, 1.0))]
    cases.append(make_case("hover_zero_velocity_yaw_held", params(0.3, 1, ROTORS), recs, [0, 1, None], init_yaw=0.7))
    # repeated early arrivals until the ring is full
    recs = [curved_record(rng, stamp(t0, k) - 2.0, 8, 0.8) for k in range(4)]
    cases.append(make_case("repeated_early_overflow", params(1.2), recs, [0, 1, 2, 3]))
    # getYaw's leaves: turn first (saturated steps from an exact init_yaw), track afterwards; both constant sets
    yaw_cases = (("yaw_A_turn_wrap_launched", LAUNCHED, -3.1, 3.1), ("yaw_A_take_launched", LAUNCHED, -3.135, 3.14),
                 ("yaw_B_turn_wrap_launched", LAUNCHED, 3.1, -3.1), ("yaw_B_take_launched", LAUNCHED, 3.135, -3.14),
                 ("yaw_C_down_launched", LAUNCHED, 0.4, 0.1), ("yaw_C_up_launched", LAUNCHED, -0.2, 0.15),
                 ("yaw_C_up_rotors", ROTORS, 0.5, 0.50913), ("yaw_C_down_rotors", ROTORS, -1.0, -1.01087),
                 ("yaw_A_turn_wrap_rotors", ROTORS, -3.138, 3.139), ("yaw_B_turn_wrap_rotors", ROTORS, 3.137, -3.14),
                 ("yaw_A_take_rotors", ROTORS, -3.1413, 3.1414), ("yaw_B_take_rotors", ROTORS, 3.1414, -3.1413))
    for name, const, init_yaw, heading in yaw_cases:
        recs = [line_record(stamp(t0, 0), (0.0, 0.0, 1.0), heading, 1.3, 2, 0.8, vz=0.05)]
        cases.append(make_case(name, params(0.3, 1, const), recs, [0, None], init_yaw=init_yaw))
    return cases


def main():
    cases = build_cases()
    near, leaves, branches, min_vxy = 0, set(), set(), math.inf
    for c in cases:
        s, b = run_case(c)
        near += s.near
        leaves |= s.leaves
        branches |= b
        min_vxy = min(min_vxy, s.min_vxy)
        print(f"{c['name']:44s} {len(c['commands']):4d} commands  size {c['final']['size']:3d}  overflow "
              f"{c['final']['overflow']}  near {s.near}  {' | '.join(c.get('branches', []))}")
    want_leaves = {"A.turn", "A.turn.wrap", "A.take", "B.turn", "B.turn.wrap", "B.take", "C.down", "C.up", "C.track", "C.hold"}
    want_branches = {"reset", "merge", "early", "early(k<0)", "silent", "held", "pop", "pop,tq<ts", "pop,t>duration"}
    assert leaves >= want_leaves, want_leaves - leaves
    assert branches >= want_branches, want_branches - branches
    assert any("merge k=118" in b for c in cases for b in c.get("branches", [])), "no merge with k = 118"
    assert any(c["final"]["overflow"] for c in cases)
    assert min_vxy >= 1e-3, min_vxy
    if near:
        raise SystemExit(f"{near} value-dependent decisions within {EPS} of their threshold: choose other seeds")
    out = {"queue": QUEUE, "near_threshold": near, "min_vxy": min_vxy, "leaves": sorted(leaves),
           "branches": sorted(branches), "cases": cases}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traj_server_independent.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {path}: {len(cases)} cases, {sum(len(c['commands']) for c in cases)} commands, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
