"""Batched replan tick driver: the per-tick data flow of the reference swarm, agents sharded over
ranks (one process per GPU).

Per tick and per agent the reference does: map update from the latest cloud + GT state
(FakeParticleRiskVoxel::updateMap incl. the neighbour overlay), BaselinePlanner::replan, then
publishes its BezierTraj on /broadcast_traj (plan_manager/src/plan_manager.cpp:364-399) which every
other agent stores (ParticleATC::trajectoryCallback, traj_coordinator/src/particles.cpp:131-191).
Here: one `sogm_update_gt` + `sogm_project_neighbours` + `sogm_replan` over the rank's agents, then
ONE all-gather of the fixed-size trajectory records (RCCL over xGMI through torch.distributed)
replaces the ROS broadcast; latest-wins per drone_id, a failed replan keeps the previous trajectory.
The replan start state is sampled from the agent's own previous trajectory at t_start
(plan_manager.cpp:169-175); agents without a trajectory hover at their position.
"""
import os

# sogm_replan runs agent groups on separate HIP streams; streams beyond the number of hardware
# queues share a queue and serialise, so ask the runtime for more queues before HIP initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

import numpy as np
import torch

from . import _abi, config, scene as scene_mod
from .planner import SogmPlanner, traj_eval
from .sogm import SogmMap, World, WorldTimelineDev, _dev, _stream, upload_scene

TICK_PERIOD = 0.1        # fsm/replan_duration (sim_fake.yaml:7)
REPLAN_START_TIME = 0.02  # fsm/replan_start_time (sim_fake.yaml:8)


def shard_bounds(rank, world, agents_per_rank):
    """Contiguous block of agents owned by `rank` (agents are the sharding axis, SURVEY §8 e)."""
    return rank * agents_per_rank, (rank + 1) * agents_per_rank


def exchange_records(own, all_records, dist, world):
    """The trajectory broadcast of the reference (/broadcast_traj, plan_manager.cpp:364-399 ->
    particles.cpp:131-191) as ONE all-gather of fixed-size records.  `own` [A_loc, 2064] uint8,
    `all_records` [A_loc * world, 2064] uint8.  Backend nccl == RCCL on ROCm; gloo on CPU tests."""
    if dist is not None and (world > 1 or dist.is_initialized()):
        dist.all_gather_into_tensor(all_records, own.contiguous())
    else:
        all_records.copy_(own)
    return all_records


class RecordExchange:
    """The same all-gather behind the C ABI (sogm_traj_allgather: ncclAllGather on the context's exchange
    stream, consumers wait for it inside the library) — what a C++ host linking libsogm_hip.so uses.  Taken when
    torch.distributed runs on RCCL (backend "nccl"); the communicator is created through sogm_comm_* with the
    128-byte id broadcast from rank 0 (dist.broadcast_object_list, like ncclGetUniqueId + MPI_Bcast in an MPI host).
    Anything else (gloo on CPU tests, no process group) uses exchange_records() above; if the communicator cannot be
    created the fallback is torch.distributed's own all-gather and `self.fallback_reason` says why (bench.py prints
    it: never silent).  `lib` / `backends` / `stream` are injection points for the CPU test, which runs this class
    against a stub library at world size 2 (tests/test_driver_gloo.py)."""

    def __init__(self, ctx, dist, rank, world, device, lib=None, backends=("nccl",), stream=None):
        import ctypes as C
        import sys
        self.ctx, self.comm, self.handle, self.fallback_reason = ctx, C.c_void_p(), None, None
        self._stream = stream if stream is not None else _stream
        self.lib = None
        if not (dist is not None and dist.is_initialized() and dist.get_backend() in backends):
            return
        if os.environ.get("SOGM_EXCHANGE", "abi") != "abi":
            self.fallback_reason = "SOGM_EXCHANGE != abi"
            return
        self.lib = lib if lib is not None else _abi.lib()
        ident = [None]
        if rank == 0:
            buf = C.create_string_buffer(_abi.SOGM_COMM_ID_BYTES)
            rc = self.lib.sogm_comm_unique_id(buf)
            ident = [buf.raw if rc == 0 else rc]
        dist.broadcast_object_list(ident, src=0)   # every rank takes part, whatever rank 0 got
        rc = ident[0] if isinstance(ident[0], int) else self.lib.sogm_comm_create(
            ident[0], rank, world, device, C.byref(self.comm))
        # all ranks must agree on the path: one failed communicator sends everybody to the fallback
        flags = [None] * world
        dist.all_gather_object(flags, int(rc))
        if any(f != 0 for f in flags):
            if rc == 0:
                self.lib.sogm_comm_destroy(self.comm)
            self.comm, self.fallback_reason = C.c_void_p(), f"sogm_comm_create returned {flags} (per rank)"
            print(f"[sogm] rank {rank}: RCCL communicator through the C ABI unavailable: {self.fallback_reason}; "
                  "using torch.distributed's all-gather", file=sys.stderr)
            return
        self.handle = self.lib.sogm_comm_handle(self.comm)

    @property
    def active(self):
        return self.handle is not None

    def info(self):
        """{ranks, rank} as RCCL itself reports them for the communicator (ncclCommCount / ncclCommUserRank)."""
        import ctypes as C
        out = (C.c_int32 * 2)()
        _abi.check(self.lib.sogm_comm_info(self.comm, out), "sogm_comm_info")
        return {"ranks": int(out[0]), "rank": int(out[1])}

    def all_gather(self, own, all_records):
        _abi.check(self.lib.sogm_traj_allgather(self.ctx, self.handle, own.data_ptr(), own.shape[0],
                                                all_records.data_ptr(), self._stream()), "sogm_traj_allgather")

    def wait(self):
        """Make torch's current stream wait for an all-gather in flight (before torch ops read the records)."""
        _abi.check(self.lib.sogm_exchange_wait(self.ctx, self._stream()), "sogm_exchange_wait")

    def close(self):
        if self.comm:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            self.lib.sogm_comm_destroy(self.comm)
            self.comm = None
            self.handle = None


class LoopbackHub:
    """Several ranks of ONE swarm flown by one process on one device, one rank after the other within a tick (bench.py's
    configs[3] rank share; tests/test_rank_share_gpu.py): stands where the collective stands.  Each rank's SwarmTick
    gets hub.exchange(rank); its all_gather() only STAGES the rank's rows, and hub.commit() — called once every
    co-simulated rank has stepped tick k — writes every staged row block into every rank's table.  So the table a rank
    reads during tick k is ver(k - 1) of all co-simulated ranks, exactly what the all-gather leaves behind
    (plan_manager.cpp:364-399 -> particles.cpp:131-191, one tick stale); rows of ranks that are not co-simulated stay
    empty records ("nothing received from that drone yet")."""

    def __init__(self, world, agents_per_rank):
        self.world, self.A_loc, self.staged = world, agents_per_rank, {}

    def exchange(self, rank):
        return _LoopbackExchange(self, rank)

    def commit(self, replayed=None):
        """`replayed`: {rank: rows} of ranks that are not flown live this time — their rows of this tick from an earlier
        pass (tools/bench_rank_share.py: one process cannot hold three planners' streams without sharing hardware
        queues, so one ring neighbour flies live and the other is replayed)."""
        rows = {s: own for s, (own, _) in self.staged.items()}
        rows.update(replayed or {})
        for _, (_, table) in self.staged.items():
            for s, own in rows.items():
                lo, hi = shard_bounds(s, self.world, self.A_loc)
                table[lo:hi].copy_(own)
        self.staged = {}


class _LoopbackExchange:
    active, fallback_reason = True, None

    def __init__(self, hub, rank):
        self.hub, self.rank = hub, rank

    def info(self):
        return {"ranks": self.hub.world, "rank": self.rank}

    def all_gather(self, own, all_records):
        self.hub.staged[self.rank] = (own, all_records)

    def wait(self):
        pass

    def close(self):
        pass


def merge_latest(new, old, ok):
    """latest-wins per drone (particles.cpp:179-190); a failed replan keeps the previous trajectory
    (the FSM keeps executing it, plan_manager.cpp:176-196)."""
    return torch.where(ok.bool().unsqueeze(1), new, old)


# ---- FiniteStateMachine::FSMCallback, per-agent state machines as tensors ----------------
FSM_NEW_PLAN, FSM_EXEC_TRAJ, FSM_REPLAN, FSM_GOAL_REACHED = 0, 1, 2, 3
REPLAN_MAX_FAILURES = 5      # fsm/replan_max_failures (sim_fake.yaml:10)
COLLI_CHECK_DURATION = 0.2   # fsm/colli_check_duration (sim_fake.yaml:9)
GOAL_TOLERANCE = 1.0         # fsm/goal_tolerance (sim_fake.yaml:5)


def hover_records(drone_ids, start_time, pos):
    """publishEmptyTrajectory (plan_manager/src/plan_manager.cpp:404-424): one 0.5 s piece whose five control
    points all sit at the current position.  Returns uint8 [n, 2064] in SogmTrajRecord layout."""
    n, dev = pos.shape[0], pos.device
    dur = torch.zeros((n, _abi.SOGM_MAX_PIECES), dtype=torch.float64, device=dev)
    dur[:, 0] = 0.5
    cpts = torch.zeros((n, _abi.SOGM_MAX_PIECES * 15), dtype=torch.float64, device=dev)
    cpts[:, :15] = pos.to(torch.float64).repeat(1, 5)
    head = torch.stack([drone_ids.to(torch.int32), torch.ones_like(drone_ids, dtype=torch.int32)], dim=1)
    parts = [head.contiguous().view(torch.uint8).view(n, 8),
             start_time.to(torch.float64).contiguous().view(torch.uint8).view(n, 8),
             dur.view(torch.uint8).view(n, -1), cpts.view(torch.uint8).view(n, -1)]
    return torch.cat(parts, dim=1)


def fsm_plan_inputs(status, traj_start, now):
    """Which agents plan in this FSM tick and from which time (plan_manager.cpp:110-135,165-175):
    NEW_PLAN plans from `now` once a second, REPLAN from now + replan_start_time."""
    is_new, is_rep = status == FSM_NEW_PLAN, status == FSM_REPLAN
    due_new = is_new & ((now - traj_start) > 1.0)
    t_start = torch.where(is_rep, now + REPLAN_START_TIME, now)
    return due_new, is_rep, t_start


def fsm_apply(status, fail, traj_start, success, now, due_new, is_rep, ok, safe, reached):
    """State update of one FSMCallback per agent (plan_manager.cpp:92-233) given this tick's replan results.
    Returns (status, fail, traj_start, success, publish_new, publish_hover, hover_start).  `safe` is isTrajSafe,
    `reached` isGoalReached; both are only consulted in EXEC_TRAJ."""
    ok = ok.bool()
    is_new, is_exec = status == FSM_NEW_PLAN, status == FSM_EXEC_TRAJ
    # NEW_PLAN (:110-135)
    traj_start = torch.where(due_new, now, traj_start)
    success = torch.where(due_new, ok, success.bool())
    pub_new = due_new & ok
    pub_hover = due_new & ~ok
    hover_start = traj_start.clone()
    st = torch.where(is_new & success, torch.full_like(status, FSM_EXEC_TRAJ), status)
    # REPLAN (:164-199)
    t_rep = now + REPLAN_START_TIME
    traj_start = torch.where(is_rep, t_rep, traj_start)
    ok_rep = is_rep & ok
    fail = torch.where(ok_rep, torch.zeros_like(fail), torch.where(is_rep, fail + 1, fail))
    pub_new = pub_new | ok_rep
    st = torch.where(ok_rep, torch.full_like(status, FSM_EXEC_TRAJ), st)
    over = is_rep & ~ok & (fail > REPLAN_MAX_FAILURES)
    st = torch.where(over, torch.full_like(status, FSM_NEW_PLAN), st)
    pub_hover = pub_hover | over
    hover_start = torch.where(over, t_rep, hover_start)
    traj_start = torch.where(over, now - 1.0, traj_start)  # force a new plan on the next tick
    # EXEC_TRAJ (:137-162)
    lapse = is_exec & ((now - traj_start) > TICK_PERIOD)   # fsm/replan_duration
    st = torch.where(lapse | (is_exec & ~safe.bool()), torch.full_like(status, FSM_REPLAN), st)
    st = torch.where(is_exec & reached.bool(), torch.full_like(status, FSM_GOAL_REACHED), st)
    return st, fail, traj_start, success, pub_new, pub_hover, hover_start


class HipCompute:
    """The rank's kernels behind the C ABI: the four calls one tick of SwarmTick.step() makes.  The product path.
    (tests/test_driver_gloo.py runs the same SwarmTick.step() over gloo on CPU with the oracle standing in for this
    class — the rank-local bookkeeping around these calls is what that test covers.)"""
    device = "cuda"

    def __init__(self, spec, scene, lo, hi, device, overlap_clear=True, double_buffer=None, grids=None, tuning=None,
                 moving_world=None, device_world=None, world_pool=None):
        half = (spec.L // 2) * 0.15
        A_loc = hi - lo
        loc = dict(scene)
        loc["n_agents"] = A_loc
        for k in ("starts", "goals", "poses", "stamps", "ego_ids"):
            loc[k] = scene[k][lo:hi]
        torch.cuda.set_device(device)
        # World frames (moving_world True / False): every tick's update takes the sensor frame OF THAT TICK (the whole
        # cloud + the cylinders, scene.WorldTimeline) and crops it on the device around each agent's current map centre
        # (sogm_update_world).  None: the frozen scene of the earlier rounds with host-side crops cut once around the
        # start (sogm_update_gt_swarm) — kept for the tests that compare single builds.
        self.timeline = scene_mod.WorldTimeline(scene, TICK_PERIOD, moving=bool(moving_world))
        self.use_world = moving_world is not None
        self._frames = {}
        # device_world (None: the environment's SOGM_DEVICE_WORLD, default 0): the frames are WRITTEN on the device from the
        # tick-0 world (sogm_world_frames, sogm.WorldTimelineDev) into a pool of world_pool frames — no host-to-device copy
        # after tick 0, constant memory however long the run.  Needs world frames; off: the uploads below, as before.
        if device_world is None:
            device_world = os.environ.get("SOGM_DEVICE_WORLD", "0") != "0" and self.use_world
        elif device_world and not self.use_world:
            raise ValueError("HipCompute(device_world=True) needs world frames (moving_world=True / False)")
        self.device_world = bool(device_world)
        self.world_pool = int(world_pool) if world_pool is not None else 8
        self._tl_dev, self._held = None, {}
        if self.use_world:
            self.dev = upload_scene(loc, cloud=np.zeros((1, 3), np.float32), cloud_range=np.zeros((A_loc, 2), np.int32))
            self.cloud_points = 0   # (per-agent counts are the device-side crop's: sogm_map_traffic / bench)
        else:
            # each agent scans only the cloud around it (its sensing neighbourhood): map half range +
            # the distance it can fly during a run, so per-agent work does not grow with the swarm
            crop, crange = scene_mod.crop_clouds(scene, lo, hi, half + 10.0)
            self.dev = upload_scene(loc, cloud=crop, cloud_range=crange)
            self.cloud_points = int(crop.shape[0])
        self.A_loc = A_loc
        self.map = SogmMap(spec, A_loc, device)
        self.overlap_mode = self.map.set_overlap_clear(overlap_clear, double_buffer=double_buffer, grids=grids)
        if "groups=" not in os.environ.get("SOGM_TUNING", ""):
            self.map.set_tuning("groups", 8)  # the grouped-stream replan (SOGM_FLOW=0): eight agent groups (32 hardware queues)
        for k, v in (tuning or {}).items():
            self.map.set_tuning(k, v)
        self.planner = SogmPlanner(self.map, config.make_astar_params(), config.make_planner_params(True),
                                   config.make_qp_settings())
        self.ego_ids = self.dev["ego_ids"]
        self.fused_update = os.environ.get("SOGM_FUSED_UPDATE", "1") != "0"

    def world(self, k):
        """The device copy of tick k's sensor frame (uploaded on first use; prepare() uploads a range ahead of a timed
        region so that no host-to-device copy falls inside it).  A frozen world has one frame."""
        key = k if self.timeline.moving else 0
        if self.device_world:
            w = self._held.get(key)
            return w if w is not None and w.tick == key else self._write_frames(key, 1)[0]
        w = self._frames.get(key)
        if w is None:
            f = self.timeline.frame(key)
            if "rings" in f:
                arr, n = self.timeline.records(key)
                w = self._frames[key] = World(f["cloud"], arr, n_cyl=n)
            else:
                w = self._frames[key] = World(f["cloud"], f["cylinders"])
        return w

    def _timeline_dev(self, n):
        """the device timeline, its pool holding at least n frames (tick 0 is uploaded on first use)"""
        if self._tl_dev is None:
            self._tl_dev = WorldTimelineDev.from_timeline(self.timeline, pool=max(self.world_pool, n))
        self._tl_dev.reserve(n)
        return self._tl_dev

    def _write_frames(self, k0, n):
        tl = self._timeline_dev(n)
        out = tl.frames(k0, n)
        self._held = {s.tick: s for s in tl._slots if s.tick is not None}
        return out

    def frames(self, k0, n):
        """The frames of ticks k0 .. k0 + n - 1 (a flight's).  device_world: ONE batched sogm_world_frames call; the pool
        grows to n if it is smaller, so that it holds the frames of a flight in the air."""
        if not self.device_world:
            return [self.world(k0 + i) for i in range(n)]
        if not self.timeline.moving:
            return [self.world(0)] * n
        held = [self._held.get(k0 + i) for i in range(n)]
        if all(w is not None and w.tick == k0 + i for i, w in enumerate(held)):
            return held
        return self._write_frames(k0, n)

    def prepare(self, k0, k1):
        if self.device_world:   # the pool and the tick-0 upload; the frames themselves are written where they are used
            self._timeline_dev(1)
            torch.cuda.synchronize()
            return
        for k in range(k0, k1):
            self.world(k)
        torch.cuda.synchronize()

    def forget(self, before):
        """drop the uploaded frames of ticks < before (device_world: nothing to drop, the pool's slots are reused)"""
        for k in [k for k in self._frames if k < before and self.timeline.moving]:
            del self._frames[k]

    @property
    def ctx(self):
        return self.map.ctx

    def set_swarm(self, all_records, A_tot, now):
        self.planner.setSwarm(all_records, A_tot, self.ego_ids, now)

    def set_swarm_views(self, views, A_tot, now):
        """set_swarm with every agent's own table (links.LinkModel.views)"""
        self.planner.set_swarm_views(views, A_tot, self.ego_ids, now)

    def update_map_views(self, poses, now, views, A_tot, tick=0):
        """update_map whose closing overlay reads every agent's own table"""
        d = self.dev
        if self.use_world:
            self.map.updateWorldViews(self.world(tick), poses, now, views, A_tot, self.ego_ids)
        else:
            self.map.updateMap(d["cloud"], d["cloud_range"], d["cylinders"], d["n_cyl"], poses, now)
            self.map.addOtherAgentsViews(views, A_tot, self.ego_ids)

    def set_publish(self, own, next_table):
        """replan() merges the new records into `own` (latest wins) and writes every agent's current record into
        `next_table` itself (sogm_planner_set_publish) — no merge launch after the replan"""
        self.planner.setPublish(own, next_table)

    def tick_inputs(self, own, stamp, hover, now, t_start, pva, poses):
        """start states from the executed trajectories, stamps and map centres: one launch (sogm_tick_inputs)"""
        _abi.check(_abi.lib().sogm_tick_inputs(own.data_ptr(), self.A_loc, stamp, REPLAN_START_TIME, hover.data_ptr(),
                                               now.data_ptr(), t_start.data_ptr(), pva.data_ptr(), poses.data_ptr(),
                                               _stream()), "sogm_tick_inputs")

    def update_map(self, poses, now, all_records, A_tot, tick=0):
        """updateMap incl. its closing neighbour overlay in one call, from the sensor frame of `tick`"""
        d = self.dev
        if self.use_world:
            self.map.updateWorld(self.world(tick), poses, now, all_records, A_tot, self.ego_ids)
        elif self.fused_update:
            self.map.updateMapSwarm(d["cloud"], d["cloud_range"], d["cylinders"], d["n_cyl"], poses, now,
                                    all_records, A_tot, self.ego_ids)
        else:  # the two separate calls (SOGM_FUSED_UPDATE=0: A/B aid)
            self.map.updateMap(d["cloud"], d["cloud_range"], d["cylinders"], d["n_cyl"], poses, now)
            self.map.addOtherAgents(all_records, A_tot, self.ego_ids)

    def set_prestamp(self, next_stamp, hover, now, t_start, pva, poses, tick=0):
        """the replan about to run (tick `tick`) also builds the NEXT tick's map and start states
        (sogm_planner_set_prestamp) — from the newest sensor frame that exists while it runs, its own tick's: the next
        tick then plans on a map whose obstacle data is one tick old (staleness 1; a frozen world hides the difference)"""
        d = self.dev
        if self.use_world:
            self.planner.setPrestamp(None, None, None, 0, next_stamp, REPLAN_START_TIME, hover, now, t_start, pva, poses,
                                     world=self.world(tick))
        else:
            self.planner.setPrestamp(d["cloud"], d["cloud_range"], d["cylinders"], d["n_cyl"], next_stamp,
                                     REPLAN_START_TIME, hover, now, t_start, pva, poses)

    def prestamp_pending(self):
        return self.map.prestamp_pending()

    def update_prestamped(self, all_records, A_tot):
        """the update of a pre-stamped tick: grid swap + neighbour overlay"""
        self.map.updatePrestamped(all_records, A_tot, self.ego_ids)

    def replan(self, pva, goals, t_start, new, ok):
        # a dataflow replan whose device-side waits timed out reports ok = 0 for the agents it could not finish and
        # counts the tick in pinned memory: a flight must not go on merging records past such a tick
        code, n = self.planner.flow_failures()
        if n:
            raise RuntimeError(f"sogm_replan: {n} tick(s) failed on the device (flow error code {code})")
        self.planner.replan(pva, goals, t_start, self.ego_ids, new, ok)

    def merge_latest(self, new, ok, own, all_records):
        """latest-wins in one launch; `all_records` (single process only) refreshes the swarm table as well"""
        _abi.check(_abi.lib().sogm_merge_latest(new.data_ptr(), ok.data_ptr(), own.data_ptr(),
                                                all_records.data_ptr() if all_records is not None else None,
                                                self.A_loc, _stream()), "sogm_merge_latest")

    def close(self):
        self.planner.close()
        self.map.close()


class SwarmTick:
    def __init__(self, grid="cfg2", agents_per_rank=None, rank=0, world=1, device=0, seed=0x5069,
                 spec=None, scene=None, dist=None, overlap_clear=True, deconflict=True, fsm=False,
                 double_buffer=None, grids=None, compute=None, exchange=None, prestamp=None, tuning=None,
                 moving_world=None, neighbour_lag=1, audit=False, device_fsm=False, traj_server=None, device_world=None,
                 world_pool=None, n_rings=0, link=None, msg_noise=None, belief=False):
        self.rank, self.world, self.dist = rank, world, dist
        # msg_noise (an _abi.SogmTrajNoise, or links.parse_noise's text): what every sender broadcasts is its executed record
        # with a localisation bias, a clock offset and a tracking error on it (include/sogm_abi.h "message noise"); the table
        # every agent executes, the audit and the trajectory server stay the true one.  belief=True: after each delivery every
        # receiver's view is scored against that true table at the tick's stamp ("belief audit"; belief_report()).  Both ride
        # on the link model and keep its restrictions; without link they fly perfect links.
        asked = "link" if link is not None else "msg_noise" if msg_noise is not None else "belief"   # named in the refusals
        if (msg_noise is not None or belief) and link is None:
            from . import links as links_mod
            link = links_mod.make_params()
        # link (an _abi.SogmLinkParams, or links.parse_params' text): every agent reads its OWN table of the swarm, what a
        # radio link with per-message delay, loss and range delivered to it (links.LinkModel; include/sogm_abi.h "radio
        # links") — on the plain lock-step path of step() and on step_fsm_device().  The audit and the trajectory server
        # keep reading the true table.  Single process, no fused publication, no pre-stamp, no flights.
        if link is not None:
            if world > 1 or (dist is not None and dist.is_initialized()):
                raise ValueError(f"SwarmTick({asked}=...) is single-process: every receiver's links are modelled in one place")
            if fsm and not device_fsm:
                raise ValueError(f"SwarmTick({asked}=...) with fsm=True needs device_fsm=True")
            if int(neighbour_lag) != 1:
                raise ValueError(f"SwarmTick({asked}=...) needs neighbour_lag=1: a uniform lag is the link's delay_min = delay_max")
            if compute is not None and not hasattr(compute, "update_map_views"):
                raise ValueError(f"SwarmTick({asked}=...) needs a compute with per-agent tables")
            prestamp = False
        # neighbour_lag = 2: the overlay and isSafeAfterOpt of tick k read table ver(k - 2) instead of ver(k - 1) — the
        # staleness rule of sogm_flight_run, flown here lock-step (one tick after the other) through the per-tick entry
        # points: the reference path the flight's records are held to, bit for bit (single process, no fused publication)
        self.neighbour_lag = int(neighbour_lag)
        assert self.neighbour_lag in (1, 2)
        self.spec = spec if spec is not None else config.make_spec(grid)
        self.A_loc = agents_per_rank if agents_per_rank is not None else config.AGENTS.get(grid, 4)
        self.A_tot = self.A_loc * world
        half = (self.spec.L // 2) * 0.15
        # n_rings > 0: the scene also has that many ring obstacles (scene.make_scene); the audit then audits them
        self.scene = scene if scene is not None else scene_mod.make_scene(self.A_tot, half, seed=seed, n_rings=int(n_rings))
        lo, hi = shard_bounds(rank, world, self.A_loc)
        if world > 1 and compute is None and dist is not None and "flight_engines" not in (tuning or {}) \
                and "flight_exchange_units" not in (tuning or {}):
            # several ranks, one GPU each: a flight's four kernels fill every compute unit, and the collective queued behind the
            # call (SogmFlight::nccl_comm) runs kernels of its own — one 16-CU unit is left to no kernel (the map kernel gives it
            # up) so that they find room.  NOT measured on hardware: no multi-GPU box.
            tuning = dict(tuning or {}, flight_exchange_units=1, flight_map_units=3)
        self.compute = compute if compute is not None else HipCompute(
            self.spec, self.scene, lo, hi, device, overlap_clear, double_buffer, grids, tuning, moving_world, device_world,
            world_pool)
        c = self.compute
        # the HIP objects, for the bench / tools / tests that use the staged entry points beside step()
        self.map, self.planner, self.dev = getattr(c, "map", None), getattr(c, "planner", None), getattr(c, "dev", None)
        self.overlap_mode, self.cloud_points = getattr(c, "overlap_mode", 0), getattr(c, "cloud_points", 0)
        d = c.device
        self.goals = _dev(self.scene["goals"][lo:hi], np.float64, d)
        self.hover = _dev(np.concatenate([self.scene["starts"][lo:hi], np.zeros((self.A_loc, 6))], axis=1), np.float64, d)
        self.pva = torch.zeros((self.A_loc, 9), dtype=torch.float64, device=d)      # replan start states of the tick
        self.poses = torch.zeros((self.A_loc, 3), dtype=torch.float32, device=d)    # map centres of the tick
        self.t_start = torch.zeros((self.A_loc,), dtype=torch.float64, device=d)
        self.own = torch.zeros((self.A_loc, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device=d)
        self.new = torch.zeros_like(self.own)
        self.ok = torch.zeros((self.A_loc,), dtype=torch.int32, device=d)
        self.all = torch.zeros((self.A_tot, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device=d)
        # replan() ends with ParticleATC::isSafeAfterOpt against the swarm's latest trajectories
        # (baseline_fake.cpp:453-460); "now" of the check = the tick's stamp
        self.now = torch.zeros((self.A_loc,), dtype=torch.float64, device=d)
        self.deconflict = deconflict
        self.links, self.msg_noise, self.belief = None, None, bool(belief)
        if link is not None:
            from . import links as links_mod
            prm = links_mod.parse_params(link) if isinstance(link, str) else link
            self.links = links_mod.LinkModel(self.A_tot, lo, self.A_loc, prm, device=d)
            if msg_noise is not None:
                self.msg_noise = links_mod.parse_noise(msg_noise) if isinstance(msg_noise, str) else msg_noise
        if deconflict and self.links is not None:
            c.set_swarm_views(self.links.views, self.A_tot, self.now)
        elif deconflict:
            c.set_swarm(self.all, self.A_tot, self.now)
        # publication inside the replan (default; SOGM_PUBLISH=0: the separate sogm_merge_latest launch): a single
        # process alternates between two swarm tables — the replan reads one (overlay, deconfliction) and its
        # finishing kernel fills the other for the next tick
        self.publish = (os.environ.get("SOGM_PUBLISH", "1") != "0" and hasattr(c, "set_publish") and not fsm
                        and self.neighbour_lag == 1 and self.links is None)
        self._tables = [self.all, torch.zeros_like(self.all)] if self.publish else None
        # pre-stamp (default; SOGM_PRESTAMP=0 or prestamp=False: off): every replan also builds the next tick's map and
        # start states, agent by agent as their records are published; the tick's inputs are double-buffered (the replan
        # in flight reads one set)
        # With world frames the default is OFF: a pre-stamp can only be fed the frame of the tick in flight, so the map the
        # next tick plans on is one tick staler than the reference's (map_input_staleness_ticks 1 vs 0) — an opt-in variant.
        self.moving_world = moving_world
        default_on = moving_world is None
        want = (os.environ.get("SOGM_PRESTAMP", "1" if default_on else "0") != "0") if prestamp is None else bool(prestamp)
        self.prestamp = want and self.publish and hasattr(c, "set_prestamp") and self.overlap_mode >= 2
        # ticks between the sensor frame a tick's map is built from and the tick itself
        self.map_input_staleness_ticks = 1 if (self.prestamp and moving_world is not None) else 0
        self._alt = (torch.zeros_like(self.pva), torch.zeros_like(self.t_start), torch.zeros_like(self.now),
                     torch.zeros_like(self.poses)) if self.prestamp else None
        # optional closed-loop mode: every agent runs the reference's FiniteStateMachine (step_fsm)
        self.fsm = fsm
        self.status = torch.full((self.A_loc,), FSM_NEW_PLAN, dtype=torch.int32, device=d)
        self.fail = torch.zeros((self.A_loc,), dtype=torch.int32, device=d)
        self.success = torch.zeros((self.A_loc,), dtype=torch.bool, device=d)
        self.traj_start = torch.full((self.A_loc,), float(self.scene["stamps"][0]) - 2.0, dtype=torch.float64, device=d)
        self.t0 = float(self.scene["stamps"][0])
        # fsm=True, device_fsm=True: the same machines as device records behind the C ABI (fsm.FsmState, step_fsm_device);
        # the replan then plans only the agents that are due
        if device_fsm and not fsm:
            raise ValueError("SwarmTick(device_fsm=True) needs fsm=True: it chooses where the state machines run")
        self.device_fsm = bool(device_fsm)
        self.fsm_dev = None
        if self.device_fsm:
            from . import fsm as fsm_mod
            self.fsm_dev = fsm_mod.FsmState(self.A_loc, self.t0 - 2.0, fsm_mod.make_params(
                TICK_PERIOD, REPLAN_START_TIME, GOAL_TOLERANCE, 1.0, REPLAN_MAX_FAILURES), device=d)
            self.status, self.fail, self.traj_start = self.fsm_dev.status, self.fsm_dev.fail, self.fsm_dev.traj_start
        self.tick = 0
        self.n_ok_total = 0
        # several ranks (or a process group of one): the swarm table is refreshed by the all-gather, not locally
        self.distributed = dist is not None and (world > 1 or dist.is_initialized())
        self.exchange = exchange if exchange is not None else RecordExchange(c.ctx, dist, rank, world, device)
        # flight audit (audit.py): every tick's executed table, this rank's rows against all rows and the world's cylinders
        self.auditor = None
        if audit:
            from .audit import SwarmAudit
            tl = getattr(c, "timeline", None) or scene_mod.WorldTimeline(self.scene, TICK_PERIOD, moving=False)
            if getattr(tl, "rings0", None) is not None:
                self.auditor = SwarmAudit(self.A_tot, self.scene["goals"][lo:hi], self.scene["starts"], tl.records(0)[0],
                                          self.t0, agent0=lo, n_local=self.A_loc, moving=tl.moving, device=d, rings=True)
            else:
                self.auditor = SwarmAudit(self.A_tot, self.scene["goals"][lo:hi], self.scene["starts"], tl.cylinders(0),
                                          self.t0, agent0=lo, n_local=self.A_loc, moving=tl.moving, device=d)

        # trajectory server (trajserver.py): the same executed tables -> every agent's 100 Hz position commands with yaw.
        # traj_server: None / False (off), True (the launched server's parameters) or a SogmTrajServerParams
        self.server = None
        if traj_server is not None and traj_server is not False:
            from . import trajserver
            self.server = trajserver.TrajServer(self.A_tot, self.scene["starts"][lo:hi], self.t0, agent0=lo, n_local=self.A_loc,
                                                prm=None if traj_server is True else traj_server, device=d)

    def _serve_tick(self, table, received=None):
        """feed the trajectory server the table every agent executes after tick self.tick (stream-ordered); received: which
        agents published in this tick (the FSM's), None: an agent whose record's start time changed"""
        if self.server is not None:
            self.server.run(table, self.t0, self.tick, TICK_PERIOD, received=received)

    def commands(self):
        """the position commands of the last step() / fly() as a numpy structured array [A_loc][ticks * 10] (synchronises);
        None when the SwarmTick was made without traj_server"""
        return self.server.commands if self.server is not None else None

    def _audit_tick(self, table):
        """audit the table every agent executes after tick self.tick (stream-ordered)"""
        if self.auditor is not None:
            self.auditor.add(table, self.t0, self.tick, TICK_PERIOD)

    def audit_report(self):
        """the flight audit's report (synchronises); None when the SwarmTick was made without audit=True"""
        return self.auditor.report() if self.auditor is not None else None

    def set_prestamp(self, on):
        """switch the pre-stamp on / off between two ticks of a flight (bench.py's labelled variant on the same swarm)"""
        c = self.compute
        on = bool(on) and self.publish and hasattr(c, "set_prestamp") and self.overlap_mode >= 2
        if on and self._alt is None:
            self._alt = (torch.zeros_like(self.pva), torch.zeros_like(self.t_start), torch.zeros_like(self.now),
                         torch.zeros_like(self.poses))
        if not on and self.prestamp:
            torch.cuda.synchronize()
            if c.prestamp_pending():   # a grid stamped for a tick that will now be built at its own start: drop it
                self.map.prestamp_join()
            self.planner.setPrestamp(None, None, None, 0, 0.0, 0.0, None, None, None, None)
        self.prestamp = on
        self.map_input_staleness_ticks = 1 if (on and self.moving_world is not None) else 0
        return on

    def close(self):
        self.exchange.close()
        self.compute.close()

    def _exchange(self):
        """The tick's trajectory broadcast: one RCCL all-gather (behind the C ABI when available)."""
        if self.exchange.active:
            self.own = self.own.contiguous()
            self.exchange.all_gather(self.own, self.all)
        else:
            exchange_records(self.own, self.all, self.dist, self.world)

    def _publish(self):
        """End of a tick: latest-wins merge of the new records into the rank's own table (a failed replan keeps
        executing the previous trajectory, plan_manager.cpp:176-196), then the broadcast (plan_manager.cpp:364-399
        -> particles.cpp:131-191): a single process refreshes the swarm table in the same launch, several ranks
        all-gather it — the records every rank overlays on its NEXT tick are one tick stale, like the ROS topic."""
        local = not self.exchange.active and not self.distributed
        self.compute.merge_latest(self.new, self.ok, self.own, self.all if local else None)
        if not local:
            self._exchange()

    def _deliver(self):
        """with link: what tick self.tick's broadcasts and the earlier ones still in the air bring every receiver — the
        table every agent executes after this tick, sent from the tick's replan start positions (stream-ordered)"""
        if self.links is not None:
            self.links.deliver(self.tick, self.own, self.pva[:, 0:3], noise=self.msg_noise)
            if self.belief:
                self.links.audit_belief(self.own, self.now)

    def belief_report(self):
        """{name: total over the receivers and the ticks so far} of the belief audit, max_q as a maximum, plus rms_m, the
        root mean square position error of the compared samples in metres (synchronises); None without belief=True"""
        if self.links is None or not self.belief:
            return None
        out = self.links.belief()
        out["rms_m"] = (out["sum_q"] / out["samples"]) ** 0.5 / 1000.0 if out["samples"] else 0.0
        return out

    def link_counters(self):
        """{name: sum over the receivers and the ticks so far} of the link model (synchronises); None without link"""
        return self.links.totals() if self.links is not None else None

    def records_all(self):
        """The swarm's latest records for torch-side readers (waits for an all-gather in flight)."""
        if self.exchange.active:
            self.exchange.wait()
        return self.all

    def step_fsm(self):
        """One FSM tick (plan_manager.cpp:92-233) for every agent: NEW_PLAN / REPLAN agents plan, EXEC_TRAJ
        agents only check time lapse, isTrajSafe and the goal; failures are counted and after
        replan_max_failures the agent publishes a hover record and starts over.  Stream-ordered, no host sync."""
        stamp = self.t0 + self.tick * TICK_PERIOD
        now = torch.full((self.A_loc,), stamp, dtype=torch.float64, device="cuda")
        self.now.copy_(now)
        due_new, is_rep, t_start = fsm_plan_inputs(self.status, self.traj_start, now)
        pva_now, valid_now = traj_eval(self.own, now)
        pva_now = torch.where(valid_now.bool().unsqueeze(1), pva_now, self.hover)
        pva, valid = traj_eval(self.own, t_start)
        pva = torch.where(valid.bool().unsqueeze(1), pva, self.hover).contiguous()
        self.hover = torch.cat([pva_now[:, :3], torch.zeros_like(pva_now[:, 3:])], dim=1)
        if getattr(self.compute, "use_world", False):
            self.map.updateWorld(self.compute.world(self.tick), pva_now[:, :3].to(torch.float32).contiguous(), now)
        else:
            self.map.updateMap(self.dev["cloud"], self.dev["cloud_range"], self.dev["cylinders"], self.dev["n_cyl"],
                               pva_now[:, :3].to(torch.float32).contiguous(), now)
        self.map.addOtherAgents(self.all, self.A_tot, self.dev["ego_ids"])
        safe = self.map.isTrajSafe(self.own, now, COLLI_CHECK_DURATION)
        self.planner.replan(pva, self.goals, t_start, self.dev["ego_ids"], self.new, self.ok)
        reached = (pva_now[:, :3] - self.goals).norm(dim=1) < GOAL_TOLERANCE
        ok = self.ok.bool() & (due_new | is_rep)
        (self.status, self.fail, self.traj_start, self.success, pub_new, pub_hover, hover_start) = fsm_apply(
            self.status, self.fail, self.traj_start, self.success, now, due_new, is_rep, ok, safe, reached)
        hover = hover_records(self.dev["ego_ids"], hover_start, pva_now[:, :3])
        self.own = torch.where(pub_new.unsqueeze(1), self.new, torch.where(pub_hover.unsqueeze(1), hover, self.own))
        # what this FSMCallback saw and did (device tensors; tests compare them with oracle/fsm_oracle.cpp)
        self.last_fsm = {"now": stamp, "ok": ok, "safe": safe, "reached": reached, "pub_new": pub_new,
                         "pub_hover": pub_hover, "hover_start": hover_start, "t_start": t_start, "pos": pva_now[:, :3]}
        self._exchange()
        if self.auditor is not None or self.server is not None:
            table = self.own if self.A_loc == self.A_tot and not self.distributed else self.records_all()
            self._audit_tick(table)
            self._serve_tick(table, pub_new | pub_hover)
        self.tick += 1
        return ok.to(torch.int32)

    def step_fsm_device(self):
        """step_fsm with the machines on the device: sogm_fsm_inputs -> map update -> overlay -> isTrajSafe -> replan of
        the agents that are due (sogm_planner_set_due) -> sogm_fsm_apply -> exchange / audit.  Same records, states and
        masked ok as step_fsm, tick for tick; the searches, corridors and QPs of EXEC_TRAJ / GOAL_REACHED agents, whose
        results step_fsm throws away, are not run.  Stream-ordered, no host sync.
        last_fsm differs from step_fsm's in two ways: "reached", "due", "hover_start", "t_start" and "pos" are the
        tick's device buffers themselves, rewritten by the next step() (clone what must outlive it; "ok" and the "pub_*"
        flags and "safe" are fresh tensors), and "hover_start" is 0 where no hover record was published (step_fsm leaves
        traj_start there); it also has "due" (sogm_fsm_inputs' bits)."""
        stamp = self.t0 + self.tick * TICK_PERIOD
        f, ego = self.fsm_dev, self.dev["ego_ids"]
        f.inputs(self.own, self.goals, stamp, self.hover, self.now, self.t_start, self.pva, self.poses)
        if getattr(self.compute, "use_world", False):
            self.map.updateWorld(self.compute.world(self.tick), self.poses, self.now)
        else:
            self.map.updateMap(self.dev["cloud"], self.dev["cloud_range"], self.dev["cylinders"], self.dev["n_cyl"],
                               self.poses, self.now)
        if self.links is not None:
            self.map.addOtherAgentsViews(self.links.views, self.A_tot, ego)
        else:
            self.map.addOtherAgents(self.all, self.A_tot, ego)
        safe = self.map.isTrajSafe(self.own, self.now, COLLI_CHECK_DURATION)
        self.planner.set_due(f.due)
        self.planner.replan(self.pva, self.goals, self.t_start, ego, self.new, self.ok)   # ok = 0 where not due
        f.apply(self.ok, safe, self.new, ego, self.own, stamp)
        ok = self.ok.clone()  # self.ok is rewritten by the next tick
        # what this FSMCallback saw and did, as step_fsm reports it; "reached", "due", "hover_start", "t_start" and "pos"
        # are the live buffers that the next tick rewrites, not copies: a reader that keeps them over a step() clones them
        self.last_fsm = {"now": stamp, "ok": ok, "safe": safe, "reached": f.reached, "due": f.due,
                         "pub_new": f.pub == _abi.FSM_PUB_NEW, "pub_hover": f.pub == _abi.FSM_PUB_HOVER,
                         "hover_start": f.hover_start, "t_start": self.t_start, "pos": f.pos_now}
        self._exchange()
        self._deliver()
        if self.auditor is not None or self.server is not None:
            table = self.own if self.A_loc == self.A_tot and not self.distributed else self.records_all()
            self._audit_tick(table)
            self._serve_tick(table, f.pub != _abi.FSM_PUB_NONE)
        self.tick += 1
        return ok

    def step(self):
        """One replan tick for every agent of this rank.  Everything is stream-ordered on the GPU."""
        if self.device_fsm:
            return self.step_fsm_device()
        if self.fsm:
            return self.step_fsm()
        stamp = self.t0 + self.tick * TICK_PERIOD
        c = self.compute
        if self.prestamp and c.prestamp_pending():
            # the previous replan built this tick's map and start states (into the alternate buffers)
            (self.pva, self.t_start, self.now, self.poses), self._alt = self._alt, (self.pva, self.t_start, self.now,
                                                                                    self.poses)
            c.update_prestamped(self.all, self.A_tot)
        else:
            c.tick_inputs(self.own, stamp, self.hover, self.now, self.t_start, self.pva, self.poses)
            if self.links is not None:
                c.update_map_views(self.poses, self.now, self.links.views, self.A_tot, self.tick)
            else:
                c.update_map(self.poses, self.now, self.all, self.A_tot, self.tick)
        if self.publish:
            local = not self.exchange.active and not self.distributed
            nxt = self._tables[(self.tick + 1) & 1] if local else None
            c.set_publish(self.own, nxt)
            if self.deconflict:
                c.set_swarm(self.all, self.A_tot, self.now)
            if self.prestamp:
                c.set_prestamp(self.t0 + (self.tick + 1) * TICK_PERIOD, self.hover, self._alt[2], self._alt[1],
                               self._alt[0], self._alt[3], self.tick)
            c.replan(self.pva, self.goals, self.t_start, self.new, self.ok)
            if local:
                self.all = nxt   # what every agent executes after this tick: the next tick's table
            else:
                self._exchange()
        elif self.neighbour_lag == 2:
            c.replan(self.pva, self.goals, self.t_start, self.new, self.ok)
            c.merge_latest(self.new, self.ok, self.own, None)   # own = ver(k)'s rows
            # self.all stays ver(k - 2) for this tick's readers; the next tick reads ver(k - 1) = the table of one tick ago
            self._lag_prev, self.all = self.own.clone(), (self._lag_prev if getattr(self, "_lag_prev", None) is not None
                                                          else torch.zeros_like(self.all))
            if self.deconflict:
                c.set_swarm(self.all, self.A_tot, self.now)
            self._audit_tick(self.own)     # ver(k); self.all is the stale table the readers see
            self._serve_tick(self.own)
        else:
            c.replan(self.pva, self.goals, self.t_start, self.new, self.ok)
            self._publish()
            self._deliver()
        if (self.auditor is not None or self.server is not None) and self.neighbour_lag == 1:
            self._audit_tick(self.records_all())
            self._serve_tick(self.records_all())
        self.tick += 1
        return self.ok.clone()  # self.ok is rewritten by the next tick

    # ---- flights: sogm_flight_run, every agent on its own clock ----
    def fly(self, n_ticks):
        """The next n_ticks ticks of every agent in ONE call (sogm_abi.h "Flight"): agent a's tick k starts when its own tick
        k - 1 is finished and every agent has finished tick k - 2; it reads the neighbours' records of tick k - 2.  Needs
        world frames (moving_world True / False) and a flight flown from tick 0 through fly() only.  Returns (ok [n, A]
        int32, records uint8 [n, A, 2064]) device tensors — valid once the stream has run the flight.
        With fsm=True, device_fsm=True every agent-tick is one FSMCallback (sogm_planner_set_flight_fsm): only the agents
        that are due replan, ok / records are the replan's outputs behind the due gate, self.status / fail / traj_start /
        own hold the state after the flight, self.flight_fsm_log the call's per-tick log (fsm.FsmState.flight_logs plus
        "ok" and "new") and self.last_fsm its last tick; with audit=True the audited tables are the log's "own".
        last_fsm after a flight has the keys "now", "ok", "safe", "reached", "due", "pub_new", "pub_hover" and
        "hover_start" — step_fsm_device's without "t_start" and "pos", which the head of a flight's tick keeps in the
        planner's own per-agent arrays and SogmFlightFsm does not log."""
        c = self.compute
        if self.links is not None:
            raise ValueError("fly() with link, msg_noise or belief: a flight reads its own ring of tables; fly step() ticks instead")
        assert getattr(c, "use_world", False), "fly() needs world frames (moving_world=True / False)"
        # the closed loop flies with the machines on the device only (sogm_planner_set_flight_fsm); the torch machines of
        # fsm=True, device_fsm=False have no flight
        assert not self.fsm or self.device_fsm
        if self.device_fsm and self.world > 1:
            raise NotImplementedError("fly() under the FSM over several ranks: fly step() ticks instead")
        if self.world > 1:
            if self.auditor is not None:
                # log_r holds this rank's rows only and the four-table ring does not keep the other ranks' versions
                raise NotImplementedError("fly() with audit=True over several ranks: audit step() ticks instead")
            if self.server is not None:
                raise NotImplementedError("fly() with traj_server over several ranks: serve step() ticks instead")
            return self._fly_ranks(n_ticks)
        if not hasattr(self, "_fl_tables"):
            assert self.tick == 0, "a flight starts at tick 0 (or continues a flight)"
            self._fl_tables = torch.zeros((4, self.A_tot, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
            self._fl_next = 0
        assert self.tick == self._fl_next, "fly() continues flights only"
        assert 1 <= n_ticks <= _abi.FLIGHT_MAX_TICKS
        log_r = torch.zeros((n_ticks, self.A_loc, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
        log_ok = torch.zeros((n_ticks, self.A_loc), dtype=torch.int32, device="cuda")
        worlds = c.frames(self.tick, n_ticks)
        sided = self.auditor is not None or self.server is not None
        executed = self.own.clone() if sided else None   # the table before the call
        fsm_log = None
        if self.device_fsm:
            # every agent's tick is one FSMCallback: the machines' records are read and left in place (self.status / fail /
            # traj_start are views of them), the per-tick log of the call is kept in self.flight_fsm_log
            fsm_log = self.fsm_dev.flight_logs(n_ticks)
            self.planner.set_flight_fsm(self.fsm_dev.prm, COLLI_CHECK_DURATION, self.fsm_dev.state, fsm_log)
        try:
            self.planner.flight(worlds, self.tick, self.t0, TICK_PERIOD, REPLAN_START_TIME, self.goals,
                                self.dev["ego_ids"], self.hover, self.own, self._fl_tables, log_r, log_ok)
        finally:
            if self.device_fsm:
                self.planner.set_flight_fsm(None)   # (copied at the call: the flight in the air keeps its mode)
        if fsm_log is not None:
            # log_ok / log_r: the replan's outputs as the due gate leaves them (what step_fsm_device has in ok / new)
            fsm_log["ok"], fsm_log["new"] = log_ok, log_r
            self.flight_fsm_log = fsm_log
            self.last_fsm = {"now": self.t0 + (self.tick + n_ticks - 1) * TICK_PERIOD, "ok": log_ok[-1],
                             "safe": fsm_log["safe"][-1], "reached": fsm_log["reached"][-1], "due": fsm_log["due"][-1],
                             "pub_new": fsm_log["pub"][-1] == _abi.FSM_PUB_NEW,
                             "pub_hover": fsm_log["pub"][-1] == _abi.FSM_PUB_HOVER,
                             "hover_start": fsm_log["hover_start"][-1]}
            if self.auditor is not None:
                self.auditor.add(fsm_log["own"], self.t0, self.tick, TICK_PERIOD)   # the executed tables themselves
            self._serve_tick(fsm_log["own"], fsm_log["pub"] != _abi.FSM_PUB_NONE)
        elif sided:
            # the flight's executed tables: latest-wins merges of its log, one launch per tick, then one audit call
            tables = torch.empty((n_ticks, self.A_tot, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
            for i in range(n_ticks):
                c.merge_latest(log_r[i], log_ok[i], executed, tables[i])
            if self.auditor is not None:
                self.auditor.add(tables, self.t0, self.tick, TICK_PERIOD)
            self._serve_tick(tables)
        self.tick += n_ticks
        self._fl_next = self.tick
        self.all = self._fl_tables[(self.tick - 1) & 3]   # ver(last tick): what every agent executes now
        return log_ok, log_r

    def _fly_ranks(self, n_ticks):
        """fly() over several ranks: tick k reads the OTHER ranks' records of tick k - 2, which only an all-gather between
        two calls can deliver — so the flight goes in calls of two ticks (k, k + 1 read ver(k - 2), ver(k - 1): both
        complete before the call), each followed by the all-gather of the two versions it finished (this rank's rows of
        ver(k), ver(k + 1) to every rank).  Same records as one process flying all agents."""
        c = self.compute
        lo, hi = shard_bounds(self.rank, self.world, self.A_loc)
        if not hasattr(self, "_fl_tables"):
            assert self.tick == 0, "a flight starts at tick 0 (or continues a flight)"
            self._fl_tables = torch.zeros((4, self.A_tot, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
            self._fl_next = 0
        assert self.tick == self._fl_next, "fly() continues flights only"
        log_r = torch.zeros((n_ticks, self.A_loc, _abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
        log_ok = torch.zeros((n_ticks, self.A_loc), dtype=torch.int32, device="cuda")
        if self.exchange.active and os.environ.get("SOGM_FLIGHT_EXCHANGE", "device") == "device":
            # the exchange behind the call (SogmFlight::nccl_comm): ONE call for all ticks — per tick a device-side wait, the
            # in-place all-gather of this rank's rows and the release of the next-but-one tick's overlays are queued on the
            # context's exchange stream; no host step between ticks, every rank passes the same n_ticks
            assert 1 <= n_ticks <= _abi.FLIGHT_MAX_TICKS
            worlds = c.frames(self.tick, n_ticks)
            self.planner.flight(worlds, self.tick, self.t0, TICK_PERIOD, REPLAN_START_TIME, self.goals, self.dev["ego_ids"],
                                self.hover, self.own, self._fl_tables, log_r, log_ok, n_total=self.A_tot, agent0=lo,
                                comm=self.exchange.handle)
            self.tick += n_ticks
            self._fl_next = self.tick
            self.all = self._fl_tables[(self.tick - 1) & 3]
            return log_ok, log_r
        done = 0
        while done < n_ticks:
            n = min(2, n_ticks - done)
            worlds = c.frames(self.tick, n)
            # (flight_guard: a test that runs several ranks as threads on ONE device serialises their calls with it — two
            #  flights at once would fight for the same compute-unit partitions, each holding what the other's kernels need)
            guard = getattr(self, "flight_guard", None)
            if guard is not None:
                guard.acquire()
            try:
                self.planner.flight(worlds, self.tick, self.t0, TICK_PERIOD, REPLAN_START_TIME, self.goals, self.dev["ego_ids"],
                                    self.hover, self.own, self._fl_tables, log_r[done:done + n], log_ok[done:done + n],
                                    n_total=self.A_tot, agent0=lo)
                if guard is not None:
                    torch.cuda.current_stream().synchronize()
            finally:
                if guard is not None:
                    guard.release()
            for k in range(self.tick, self.tick + n):
                tab = self._fl_tables[k & 3]
                if self.exchange.active:
                    self.exchange.all_gather(tab[lo:hi], tab)     # in place: this rank's rows are where they belong
                    self.exchange.wait()
                else:
                    exchange_records(tab[lo:hi].clone(), tab, self.dist, self.world)
            self.tick += n
            done += n
        self._fl_next = self.tick
        self.all = self._fl_tables[(self.tick - 1) & 3]
        return log_ok, log_r
