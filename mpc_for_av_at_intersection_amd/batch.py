"""Batched closed loop: B independent intersection instances x A agents advanced in lock-step on one GPU.

One `step()` is the body of the reference's scenario loop (main/scenarios/mpc_intersection.py:95-159) for every
(instance, agent) pair: nearest index on the full path, ego prediction, prediction of the other agents, conflict
search and path cut (mpcx_interaction_batch), reference window + warm-start rollout (mpcx_mpc_prepare_batch), the
QP (mpcx_qp_solve_batch) and the plant update (mpcx_plant_step_batch). Every other agent of the same instance plays
the role of the reference's `moving_obstacles`: it is described by (x, y, v, yaw, a, steer) exactly like
`MovingObstacle*.get()` (a, steer = the controls it applied last step). An instance may also carry the reference's own
SCRIPTED cars (lib/moving_obstacles.py; `traffic=`): they are stepped on the device too (mpcx_traffic_step_batch) and share
the instance's rows of the obstacle pool with its agents. All state lives on the device.
`run(n)` hands the whole loop to mpcx_closed_loop_run (n steps enqueued back to back, optionally as a replayed
hipGraph); `step_staged()` drives the same kernels stage by stage through the per-stage entry points.
`stop_mode='speed'` is the reference's NEWER scenario script (main/scenarios/mpc_intersection_new_ref.py with lib/mpc_with_speed.py): the
path stays whole and the speed reference is zeroed from the conflict on, instead of the path being cut in front of it.
`attach_log(capacity)` adds the RUN LOG: one more kernel at the end of every step writes the reference's History row, the goal test of
its loop and the true clearance to the other vehicles, per agent, on the device (RunLog).
`retire_at_goal()` ends an agent's episode where the reference's loop ends (`if mpc.is_goal(state): break`): from the step after its
arrival on it is a parked car that is not solved, not logged and not counted; `run_until_done()` runs until every agent has arrived.
`retire_at_goal(leave_scene=True)` is DEPARTURE: the arrived car is also taken out of the scene -- from the next step on nobody's conflict
search and nobody's clearance sees it (two stock routes share every exit arm: a car parked on the goal would block the second for good).
`enter_on_schedule(wait, gap)` is ADMISSION, the counterpart: scheduled agents wait outside the scene and enter, on the device, in the step
their count-down ends -- or the first later step in which their start pose is `gap` clear of everybody present (entry_schedule() draws
seeded arrival times per approach queue).
`respawn_on_schedule(due, gap)` is RESPAWN, which makes the three an open intersection: every slot serves a stream of vehicles -- when one
arrives its episode is recorded (episodes()), the slot is reset to a fresh start and the next vehicle goes through the gate at its due step
(demand_schedule() draws seeded arrival streams per approach queue).
`respawn_on_schedule(due, gap, route=...)` gives every vehicle of a slot its OWN ROUTE (and start index): the reset also writes the slot's
`path_off` / `path_len`, so turning proportions vary per vehicle with no host work between steps (turning_demand() draws seeded routes per
approach arm; episode_routes() and movement_summary() read the run per movement, the latter reduced on the device).
`give_way(order)` is RIGHT OF WAY: every pool row has a precedence word, and an agent sees the cars whose word is larger than its own as
standing cars at their present pose -- which ends the mutual wait of yield-to-everybody at the crossing; order='entry' is first come, first
served, stamped on the device as vehicles are admitted.
`signalise(plans)` puts TRAFFIC SIGNALS on the crossing: stop lines are a property of path points (stop_lines()), a plan gives every signal
group its green within a cycle (two_phase_plan()), and one more small launch behind the conflict search holds an agent whose light is red
-- or amber, if it can still stop -- at its line by cutting its path there; a table of plans runs a sweep of timings as one batch.
`actuate(controllers)` makes the signals VEHICLE-ACTUATED: every instance is a junction with a controller on the device that holds a phase
at least its minimum green, extends it while cars approach its lines, ends it after a gap or at a maximum if somebody else waits, and skips
phases nobody calls (two_phase_controller()); the launch takes the place of the fixed plan's, the hold at the line is the same.
`advise_speed()` is SIGNAL-AWARE APPROACH SPEED for a signalised batch in speed mode: an agent that would reach its stop line on red at cruise
speed gets the speed with which it reaches the line as the light turns green as a cap on its speed reference (one launch between the
window stage and the QP); the hold stays the safety net behind it.
`reserve(managers)` runs the crossing UNSIGNALISED BY RESERVATION: every instance is a junction with a manager on the device that admits a
car only if its movement (movement_lines()) conflicts with no movement that holds the crossing (movement_conflicts()), first come, first
served; everybody else waits at its stop line.  The launch takes the place of the signals', the hold at the line is the same.
`follow()` is CAR FOLLOWING, beside every other stage and in both stop modes: every agent finds the nearest vehicle ahead on its own path
and stops a standstill distance plus a time gap behind it -- the hold at a line that moves --, in speed mode under Gipps' safe speed as a
cap on its speed reference (one launch in front of the window stage, in speed mode one behind it).
`watch_safety()` is THE NEAR-MISS LOG, beside every other stage: one launch behind the conflict search names every agent's nearest vehicle
and its first predicted contact and keeps a table of encounters on the device; near_misses() reads it, conflict_matrix() reduces it per
pair of movements.  It decides nothing.
`occlude()` is LINE OF SIGHT, beside every other stage on a scene: one launch in front of the conflict search decides which rows of its
window every agent sees (sensor range, convex occluders, connected vehicles that are heard), and the conflict search leaves the others out of
that agent's obstacle list.  corner_blocks() gives the buildings of the stock four-way world.
`keep_clear()` is KEEP CLEAR for a batch under signalise() or actuate(): one launch behind the hold keeps a car whose light lets it go at its
stop line while a movement that conflicts with its own (cross_phase_conflicts()) is inside the crossing; enter_on_green() switches it off.
`priority_road()` is the PRIORITY-CONTROLLED JUNCTION, for a batch without signals: one launch in the hold's place keeps a car of a minor
movement at its stop line until the conflicting movements of smaller rank (priority_ranks()) leave it its critical gap; all_roads_equal()
switches it off.
`stop_signs()` is the STOP-CONTROLLED JUNCTION, all-way or two-way (sign_table()), for a batch without signals: one launch in the same
place keeps a car of a signed movement at its stop line until it has stood there and the cars that stopped before it, and the unsigned
traffic within its critical gap, let it go; no_signs() switches it off.
`hold_firmly()` is the FIRM HOLD for speed mode: two small launches around the window stage make a car that signals, a reservation, keep
clear, the priority road or stop signs keep at its line really stop in front of it (the position reference ends on a stop point, a braking profile
caps the speed reference, the path index is pinned while the car is behind the line); hold_softly() switches it off.
"""
import dataclasses
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .runtime import (path_first_within, path_plan, path_tables, traffic_pool_layout, Context, InteractionParams, MpcParams, MpcxError,
                      Traffic)


RUN_LOG_DTYPE = np.dtype([(n, '<f8') for n in _lib.RUN_LOG_F64] + [(n, '<i4') for n in _lib.RUN_LOG_I32])
RUN_LOG_MAX_BYTES = 1 << 30     # attach_log refuses a larger log unless told otherwise
EPISODE_DTYPE = np.dtype([(n, '<i4') for n in ('slot', 'generation', 'due', 'entered', 'arrived', 'steps_driven', 'delay')] + [('contact', '?'),
                         ('min_clearance', '<f8'), ('row_begin', '<i4'), ('row_end', '<i4')])
MOVEMENT_DTYPE = np.dtype([(n, '<i8') for n in _lib.SUMMARY_I64] + [('min_clearance', '<f8')])
# IntersectionBatch.near_misses() and conflict_matrix(): an event of the near-miss log, a cell of the conflict matrix
NEAR_MISS_DTYPE = np.dtype([('agent', '<i4')] + [(n, '<i4') for n in _lib.SAFETY_I32] + [('min_clearance', '<f8'), ('v', '<f8'), ('ttc', '<f8')])
CONFLICT_DTYPE = np.dtype([(n, '<i8') for n in _lib.SAFETY_SUMMARY_I64] + [(n, '<f8') for n in _lib.SAFETY_SUMMARY_F64])
# IntersectionBatch.snapshot(): stage -> (key, attribute) of the device words it adds while the stage is on.  precedence: the word of every
# pool row; held: 0 free, 1 at red, 2 at amber; advised: the speed advised in the last step, 0 = none; shared_frames: frames of the agent's
# own row taken from its plan in the last step; granted, since: per agent; occupied: per junction, the movements on the crossing
_SNAPSHOT_WORDS = {'retire': (('done', 'done'), ('steps_driven', 'steps_driven')), 'scene': (('absent', 'absent'),),
                   'admit': (('wait', 'wait'), ('entered_step', 'entered_step')), 'respawn': (('served', 'served'),),
                   'precedence': (('precedence', 'prec'),), 'signals': (('held', 'held'),), 'advice': (('advised', 'advised'),),
                   'intent': (('shared_frames', 'shared_frames'),), 'reservation': (('granted', 'granted'), ('since', 'since'), ('occupied', 'occupied'))}


class RunLog:
    """The run log of an IntersectionBatch (attach_log): owns the device tensors mpcx_run_log names and reads them back.

    Per step and agent (rows): the state after the plant step, the applied controls, the reference's xref_deviation (mpc.py:301-308; NaN
    after a failed solve), the clearance to every other vehicle of the agent's pool window at the START of the step (min disc distance
    - 2 radius; +inf if there is nobody) and the step's integer decisions.  Per agent (outcomes): `steps` recorded, `goal_step` = steps
    taken when mpc.is_goal (mpc.py:310-326) first held, i.e. the reference's number of loop iterations (-1: not yet), and, counted from the
    agent's first step with clearance >= 0 on, `min_clearance` and `contact_step` (first step with clearance < 0 after that, -1 = none) --
    the stock scenario spawns a scripted car ON the ego's start pose, which a plain minimum would report as a contact at step 0.
    Nothing is frozen at the goal: the log says where the reference's loop would have ended, history() cuts there.
    With IntersectionBatch.retire_at_goal() an agent gets no row after the step of its arrival: its `steps` stops at goal_step, its
    min_clearance and contact_step stay.  rows() for all agents then has as many rows as the longest episode, and the rows of an agent
    beyond its own `steps` are zero (rows(q) is cut at that agent's own `steps`).
    Memory: 96 bytes per agent and step (capacity x P rows) + 24 bytes per agent; capacity 0 keeps the outcomes only."""

    def __init__(self, batch: 'IntersectionBatch', capacity: int, goal_dis: float, stop_speed: float):
        dev, P = batch.ctx.device, batch.P
        self.batch, self.capacity, self.goal_dis, self.stop_speed = batch, int(capacity), float(goal_dis), float(stop_speed)
        self.P, self.dt = P, float(batch.params.dt)
        self.rows_f64 = torch.zeros((self.capacity, P, 8), dtype=torch.float64, device=dev) if self.capacity else None
        self.rows_i32 = torch.zeros((self.capacity, P, 8), dtype=torch.int32, device=dev) if self.capacity else None
        self.steps, self.goal_step, self.contact_step, self.flags = (torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(4))
        self.min_clearance = torch.zeros(P, dtype=torch.float64, device=dev)
        self.c = _lib.RunLogC()
        self.c.capacity, self.c.goal_dis, self.c.stop_speed = self.capacity, self.goal_dis, self.stop_speed
        for n in ('rows_f64', 'rows_i32', 'steps', 'goal_step', 'contact_step', 'flags', 'min_clearance'):
            t = getattr(self, n)
            setattr(self.c, n, None if t is None else t.data_ptr())
        self.reset()

    @property
    def nbytes(self) -> int:
        return self.capacity * self.P * _lib.RUN_LOG_ROW_BYTES + self.P * _lib.RUN_LOG_AGENT_BYTES

    def reset(self):
        """forget everything recorded: the next step is step 0 of the log, the batch's state now is the log's initial state.  The goal
        test BEFORE that step (the top of the reference's first iteration; only a path of fewer than 5 points can pass it) is made here,
        on the host, and gives goal_step = 0."""
        b = self.batch
        b.ctx.synchronize()
        self.steps.zero_(); self.flags.zero_()
        self.contact_step.fill_(-1)
        self.min_clearance.fill_(float('inf'))
        self.initial = b.state.cpu().numpy().copy()
        path = b.path.cpu().numpy()
        off, ln = b.path_off.cpu().numpy().astype(np.int64), b.path_len.cpu().numpy().astype(np.int64)
        cut = b.inter['cut_len'].cpu().numpy().astype(np.int64)
        cut = np.where(cut > 0, cut, ln)            # len(self.cx): the full path until a step has cut it
        if b.stop_mode == 'speed':
            cut = ln                                # ... and always in speed mode (cut_len holds the stop index there)
        goal = path[off + ln - 1]
        st = self.initial
        there = ((np.hypot(st[:, 0] - goal[:, 0], st[:, 1] - goal[:, 1]) <= self.goal_dis) & (np.abs(b.target_ind.cpu().numpy() - cut) < 5) &
                 (np.abs(st[:, 2]) <= self.stop_speed))
        self.goal_step.copy_(b.ctx.i32(np.where(there, 0, -1)))
        b.ctx.synchronize()

    def outcomes(self) -> dict:
        """host arrays goal_step, contact_step, min_clearance, steps (synchronises)"""
        self.batch.ctx.synchronize()
        return {n: getattr(self, n).cpu().numpy().copy() for n in ('goal_step', 'contact_step', 'min_clearance', 'steps')}

    def rows(self, q: Optional[int] = None) -> np.ndarray:
        """the recorded rows as a structured host array (RUN_LOG_DTYPE), cut at min(steps, capacity): shape (n,) for agent q, (n, P)
        for all agents (every agent of a batch is offered the same number of rows -- unless agents are retired at their goal: then n
        is the largest `steps` and an agent's rows beyond its own `steps` are zero).  steps > capacity: the log overflowed, the first
        `capacity` rows are there."""
        self.batch.ctx.synchronize()
        steps = self.steps.cpu().numpy()
        n = min(int(steps.max() if q is None else steps[q]), self.capacity)
        shape = (n, self.P) if q is None else (n,)
        out = np.zeros(shape, RUN_LOG_DTYPE)
        if n:
            f = (self.rows_f64[:n] if q is None else self.rows_f64[:n, q]).cpu().numpy()
            w = (self.rows_i32[:n] if q is None else self.rows_i32[:n, q]).cpu().numpy()
            for k, name in enumerate(_lib.RUN_LOG_F64):
                out[name] = f[..., k]
            for k, name in enumerate(_lib.RUN_LOG_I32):
                out[name] = w[..., k]
            if q is None:       # agents retired at their goal: nothing beyond an agent's own cursor (a reused buffer may hold older rows)
                out[np.arange(n)[:, None] >= np.minimum(steps, self.capacity)[None, :]] = 0
        return out

    def history(self, q: int):
        """the reference's History of agent q (lib/simulation.py): the initial state first (a = delta = xref_deviation = 0, as
        HistorySimulation stores it), then one entry per step through History.store, cut where the reference's loop ends (goal_step
        entries after the initial one).  `t` is the class's own: store() appends current time + dt for the initial entry too, so
        t[k] = (k + 1) dt, exactly as in the reference's HistorySimulation (not k dt)"""
        from .lib.simulation import History, State
        rows = self.rows(q)
        goal = int(self.goal_step[q:q + 1].cpu()[0])       # (rows() has synchronised)
        if goal >= 0:
            if goal > len(rows):
                raise MpcxError('run log: agent %d arrived after %d steps and only %d rows were kept (capacity %d)' % (q, goal, len(rows), self.capacity))
            rows = rows[:goal]
        h = History(sample_time=self.dt)
        x, y, v, yaw = (float(c) for c in self.initial[q])
        h.store(State(x=x, y=y, yaw=yaw, v=v), a=0., delta=0., xref_deviation=0.)
        for r in rows:
            dev = float(r['xref_deviation'])
            h.store(State(x=float(r['x']), y=float(r['y']), yaw=float(r['yaw']), v=float(r['v'])), a=float(r['accel']), delta=float(r['steer']),
                    xref_deviation=None if np.isnan(dev) else dev)
        return h


class IntersectionBatch:
    def __init__(self, ctx: Context, params: MpcParams, ip: InteractionParams, routes: Sequence[np.ndarray], dl: float,
                 route_of_agent: np.ndarray, start_index: np.ndarray, v0: Optional[np.ndarray] = None,
                 tuning: Optional[np.ndarray] = None, agent_shard: Optional[tuple] = None, exchange=None,
                 pose_offset: Optional[np.ndarray] = None, traffic: Optional[Traffic] = None, stop_mode: str = 'cut',
                 v_ref: Optional[float] = None, route_speed: Optional[Sequence[np.ndarray]] = None):
        """routes: list of (n_r, 3) paths whose yaw column is already unwrapped (MPC.__init__, mpc.py:257);
        route_of_agent, start_index: integer arrays of shape (B, A); tuning: optional (B, 16) or (B*A, 16) array of
        MpcParams.tuning_row()s -- one cost/limit set per instance (or agent), the batched form of the reference's
        sensitivity sweeps (scenarios/mpc_sensitivity_analysis.py).

        agent_shard = (rank, world): the AGENT-SHARDED multi-GPU layout (sharding.py): this rank drives agents
        rank*A/world .. of EVERY instance and sees the other ranks' agents only as moving obstacles, through one
        all-gather of 6-double agent states per step.  `exchange` says who moves the rows: 'rccl' (mpcx_allgather_states
        on the context's communicator, inside mpcx_closed_loop_run) or a callable local(B, A_loc, 6) -> pool(B, A, 6)
        (sharding.torch_exchange: torch.distributed, used for gloo rehearsals).
        pose_offset: optional (B, A, 2) array (lateral offset [m] to the left of the path, heading error [rad]) added to the start
        poses, which otherwise sit exactly on the path (config2_batch).
        traffic: optional runtime.Traffic -- scripted cars per instance (scenarios/mpc_intersection.py:42-45), stepped on the device; the
        pool then holds [A agents | K actors] per instance (runtime.traffic_pool_layout).  None: exactly the ego-only batch.
        stop_mode: how an ego yields to a conflict.  'cut' (scenarios/mpc_intersection.py): its path is cut in front of the conflict.
        'speed' (scenarios/mpc_intersection_new_ref.py:90-159 + lib/mpc_with_speed.py:276-282): the path stays whole, the conflict search's
        cut index is the agent's STOP INDEX and the speed reference xref[2] is v_ref in front of it and 0 from it on (build `params` with
        lib.mpc_with_speed.params(), whose speed weight 20 tracks it).  inter['cut_len'] and the run log's cut_len column then hold the
        stop index, the path length where there is none (stop_index() gives it in the reference's own terms); the goal test is against
        the whole path.  v_ref: default lib.mpc_with_speed.MAX_SPEED.
        route_speed: optional speed profile, one array per route with one value per path point: xref[2] in front of the stop index (in
        'cut' mode: everywhere) instead of v_ref (of 0 in 'cut' mode) -- the `cv` of lib/mpc_with_speed.MPC."""
        if stop_mode not in _lib.STOP_MODES:
            raise MpcxError('unknown stop_mode %r: \'cut\' or \'speed\' (MPCX_E_INVALID)' % (stop_mode,))
        if v_ref is None:
            from .lib.mpc_with_speed import MAX_SPEED as v_ref
        if not np.isfinite(v_ref):
            raise MpcxError('v_ref = %r is not finite (MPCX_E_INVALID)' % (v_ref,))
        if route_speed is not None and (len(route_speed) != len(routes) or any(np.shape(v) != (len(r),) for v, r in zip(route_speed, routes))):
            raise ValueError('route_speed: one array per route with one value per path point expected, got lengths %s for routes of %s points'
                             % ([int(np.size(v)) for v in route_speed], [len(r) for r in routes]))
        self.stop_mode, self.v_ref = stop_mode, float(v_ref)
        # (a copy: the arc-length table below belongs to THIS batch's paths)
        ip = dataclasses.replace(ip, max_path_len=max(int(ip.max_path_len), max(len(r) for r in routes)))     # sizes the interaction kernel's LDS
        self.ctx, self.params, self.ip, self.dl = ctx, params, ip, float(dl)
        ctx.set_mpc_params(params)
        route_of_agent = np.asarray(route_of_agent, dtype=np.int64)
        start_index = np.asarray(start_index, dtype=np.int64)
        self.A_total = route_of_agent.shape[1]
        self.shard_rank, self.shard_world = (0, 1) if agent_shard is None else (int(agent_shard[0]), int(agent_shard[1]))
        self.exchange = exchange
        a_lo = 0
        if agent_shard is not None:
            if self.A_total % self.shard_world:
                raise ValueError('agent-sharded layout: %d agents do not divide over %d ranks' % (self.A_total, self.shard_world))
            if exchange is None and self.shard_world > 1:
                raise ValueError('agent-sharded layout needs an exchange (\'rccl\' or a callable)')
            a_loc = self.A_total // self.shard_world
            a_lo = self.shard_rank * a_loc
            route_of_agent = route_of_agent[:, a_lo:a_lo + a_loc]
            start_index = start_index[:, a_lo:a_lo + a_loc]
            if v0 is not None:
                v0 = np.asarray(v0, dtype=np.float64).reshape(-1, self.A_total)[:, a_lo:a_lo + a_loc]
            if pose_offset is not None:
                pose_offset = np.asarray(pose_offset, dtype=np.float64).reshape(-1, self.A_total, 2)[:, a_lo:a_lo + a_loc]
        self.B, self.A = route_of_agent.shape
        P = self.P = self.B * self.A
        T = params.T
        offs = np.cumsum([0] + [len(r) for r in routes])
        table = np.concatenate(routes, axis=0).astype(np.float64)
        self.path = ctx.f64(table)
        self._route_offs, self._route_table = offs.astype(np.int64), table      # host copies: respawn_on_schedule(route=...) looks poses up
        self.path_cs = ctx.f64(np.column_stack([np.cos(table[:, 2]), np.sin(table[:, 2])]))
        # paths are constants of the run: their arc lengths are summed once here instead of by every agent in every step (the conflict
        # search takes its resampling buckets from this table wherever that is safe, mpcx_interaction_params.path_cum)
        cum, cum_err = path_tables(table, offs)
        self.path_cum = ctx.f64(cum)
        ip.path_cum, ip.path_cum_err = self.path_cum, cum_err
        # ... and so is the answer of get_cutoff_curve_by_position_idx for every path point (the conflict search only ever asks it for one)
        self.path_first_within = ctx.i32(path_first_within(table, offs))
        ip.path_first_within = self.path_first_within
        # ... and so is the ego prediction from every path point once the predicted speed has saturated (kept poses, their discs, run boxes)
        pkey = (hash(table.tobytes()), tuple(int(o) for o in offs), float(ip.dt), float(ip.max_speed), tuple(float(v) for v in np.asarray(ip.circle_centers).ravel()),
                float(ip.radius), int(ip.pred_steps))
        pl = _PLAN_CACHE.get(pkey)
        if pl is None and len(table) * 64 * 32 > (256 << 20):
            pl = False                   # 2 KB of table per path point: beyond 256 MB the kernels resample instead (identical outputs)
        if pl is None:                   # (a few tenths of a second per set of routes: numpy over every start point of every route)
            if len(_PLAN_CACHE) > 8:
                _PLAN_CACHE.clear()
            pl = _PLAN_CACHE[pkey] = path_plan(table, np.column_stack([np.cos(table[:, 2]), np.sin(table[:, 2])]), offs, ip.dt, ip.max_speed,
                                               ip.circle_centers, ip.radius, ip.pred_steps)
        self.plan = dict(pl, cnt=ctx.i32(pl['cnt']), disc=ctx.f64(pl['disc']), box=ctx.f64(pl['box']), path_disc=ctx.f64(pl['path_disc'])) if pl else None
        ip.plan = self.plan
        r = route_of_agent.reshape(-1)
        s = start_index.reshape(-1)
        self.path_off = ctx.i32(offs[r])
        self.path_len = ctx.i32(np.array([len(routes[k]) for k in r]))
        pts = table[offs[r] + s]
        st = np.zeros((P, 4))
        st[:, 0], st[:, 1], st[:, 3] = pts[:, 0], pts[:, 1], pts[:, 2]
        if v0 is not None:
            st[:, 2] = np.asarray(v0, dtype=np.float64).reshape(-1)
        if pose_offset is not None:
            po = np.asarray(pose_offset, dtype=np.float64).reshape(P, 2)
            st[:, 0] -= np.sin(pts[:, 2]) * po[:, 0]
            st[:, 1] += np.cos(pts[:, 2]) * po[:, 0]
            st[:, 3] += po[:, 1]
        dev = ctx.device
        self.state = ctx.f64(st)
        self.applied = torch.zeros((P, 2), dtype=torch.float64, device=dev)      # (steer, accel) of the last step
        self.traj_idx = ctx.i32(s)
        self.target_ind = ctx.i32(s)
        # the obstacle pool holds ALL agents of every instance, in (instance, global agent) order; an agent skips its own row
        self.obs_off = ctx.i32(np.repeat(np.arange(self.B) * self.A_total, self.A))
        self.obs_cnt = torch.full((P,), self.A_total, dtype=torch.int32, device=dev)
        self.obs_skip = ctx.i32((np.arange(self.B)[:, None] * self.A_total + a_lo + np.arange(self.A)[None, :]).reshape(-1))
        f = torch.float64
        self.obs6 = torch.zeros((self.B * self.A_total, 6), dtype=f, device=dev)
        self.traffic = traffic
        if traffic is not None:
            # ... and, behind them, the instance's scripted actors: [A agents | K_b actors | unused up to max K]
            if self.shard_world > 1:
                raise ValueError('scripted traffic is instance-local: shard a batch that has it by instances, not by agents')
            lay = traffic_pool_layout(self.B, self.A, traffic.k_of_instance, a_lo, self.A_total)      # ValueError beyond MPCX_MAX_OBS
            self.obs_off, self.obs_cnt, self.obs_skip = ctx.i32(lay['obs_off']), ctx.i32(lay['obs_cnt']), ctx.i32(lay['obs_skip'])
            self.ego_row, self.actor_row = ctx.i32(lay['ego_row']), ctx.i32(lay['actor_row'])
            self.ego_row64 = self.ego_row.long()
            self.obs6 = torch.zeros((lay['pool_rows'], 6), dtype=f, device=dev)
            self.actors = torch.as_tensor(np.frombuffer(traffic.actors.tobytes(), dtype=np.uint8).copy()).to(dev)
            self.traffic_state = ctx.f64(traffic.state)
            self.tape = ctx.f64(traffic.tape) if traffic.tape is not None and len(traffic.tape) else None
        self.obs_local = torch.zeros((P, 6), dtype=f, device=dev) if agent_shard is not None else None
        # cut_len doubles as "length of the previous tmp_trajectory" (0 = none yet) for the next step
        # (every output is zero until a step has written it: an agent that waits to enter the scene is never stepped, and shows zeros)
        self.inter = dict(hit_idx=torch.zeros(P, dtype=torch.int32, device=dev), hit_xy=torch.zeros((P, 2), dtype=f, device=dev),
                          cut_len=torch.zeros(P, dtype=torch.int32, device=dev))
        self.pre = dict(xref=torch.zeros((P, 4, T + 1), dtype=f, device=dev),
                        reaches_end=torch.zeros((P, T + 1), dtype=torch.uint8, device=dev),
                        xbar=torch.zeros((P, 4, T + 1), dtype=f, device=dev))
        self.sol = dict(x=torch.zeros((P, 4, T + 1), dtype=f, device=dev), u=torch.zeros((P, 2, T), dtype=f, device=dev),
                        status=torch.zeros(P, dtype=torch.int32, device=dev), iters=torch.zeros(P, dtype=torch.int32, device=dev),
                        kkt=torch.zeros((P, 4), dtype=f, device=dev))
        self.steps_done = 0
        self.lin_passes = 1          # lib/mpc.py MAX_ITER: (window, rollout, QP) passes per step; the stock mpc_config.json has 1
        self.path_v = None if route_speed is None else ctx.f64(np.concatenate([np.asarray(v, dtype=np.float64) for v in route_speed]))
        # speed mode: the length of the previous step's tmp_trajectory, which the conflict search reads: 0 = none yet, then the path length
        # (mpc_intersection_new_ref.py:98,131,136).  On the device and set by the step itself: a replayed graph must see it change
        self.prev_len = torch.zeros(P, dtype=torch.int32, device=dev) if stop_mode == 'speed' else None
        self._opts = None
        if stop_mode == 'speed':
            self._opts = _lib.ClosedLoopOptsC(_lib.STOP_SPEED, 0, self.v_ref, self.prev_len.data_ptr())
        self.tuning = None
        if tuning is not None:
            tuning = np.asarray(tuning, dtype=np.float64)
            if tuning.shape == (self.B, 16):
                tuning = np.repeat(tuning, self.A, axis=0)
            elif agent_shard is not None and tuning.shape == (self.B * self.A_total, 16):
                tuning = tuning.reshape(self.B, self.A_total, 16)[:, a_lo:a_lo + self.A].reshape(-1, 16)
            if tuning.shape != (P, 16):
                raise ValueError('tuning must have shape (B, 16) or (B*A, 16)')
            self.tuning = ctx.f64(tuning)
        self._desc = None
        self.log: Optional[RunLog] = None
        self.done: Optional[torch.Tensor] = None             # retire_at_goal(): int32 (P,), != 0 = arrived and retired
        self.steps_driven: Optional[torch.Tensor] = None     # ... int32 (P,), steps taken while driving
        self._retire = None
        self.absent: Optional[torch.Tensor] = None           # retire_at_goal(leave_scene=True): int32 (pool rows,), != 0 = not in the scene
        self._scene = None
        self.wait: Optional[torch.Tensor] = None             # enter_on_schedule(): int32 (P,), -1 = in / not scheduled, > 0 steps to wait, 0 due
        self.entered_step: Optional[torch.Tensor] = None     # ... int32 (P,), the clock at the agent's admission, -1 = not yet in
        self.clock: Optional[torch.Tensor] = None            # ... int32 (1,), steps completed since enter_on_schedule()
        self.scheduled_step: Optional[np.ndarray] = None     # ... host, (P,): the step the agent was scheduled for (0 = from the start)
        self._admit = None
        self.served: Optional[torch.Tensor] = None           # respawn_on_schedule(): int32 (P,), episodes finished per slot
        self.due: Optional[torch.Tensor] = None              # ... int32 (P, G), the step at which vehicle g of slot q asks to enter
        self.ep_i32: Optional[torch.Tensor] = None           # ... int32 (P, G, 8) and float64 (P, G, 2): the episode table (_lib.EPISODE_*)
        self.ep_f64: Optional[torch.Tensor] = None
        self.start_state: Optional[torch.Tensor] = None      # ... float64 (P, 4) and int32 (P,): what a reset puts a slot back to
        self.start_idx: Optional[torch.Tensor] = None
        self._respawn = None
        self.route_of: Optional[torch.Tensor] = None         # respawn_on_schedule(route=...): int32 (P, G), the route of vehicle g of slot q
        self.route_start_state: Optional[torch.Tensor] = None    # ... float64 (P, G, 4) and int32 (P, G): every vehicle's start pose and index
        self.route_start_idx: Optional[torch.Tensor] = None
        self.route_off: Optional[torch.Tensor] = None        # ... int32 (R,) each: the routes' runs in the path tables
        self.route_len: Optional[torch.Tensor] = None
        self._routes = None
        self.prec: Optional[torch.Tensor] = None             # give_way(): int32 (pool rows,), the precedence words, a smaller word goes first
        self.stand: Optional[torch.Tensor] = None            # ... float64 (pool rows, 4), the standing records (scratch)
        self._precedence = None
        self.tick: Optional[torch.Tensor] = None             # signalise(): int32 (P,), every agent's signal clock
        self.held: Optional[torch.Tensor] = None             # ... int32 (P,), 0 free, 1 held at red, 2 held at amber
        self._signals = None
        self._signal_tabs = None                             # ... the device tables the struct names (kept alive here)
        self.junction_state: Optional[torch.Tensor] = None   # actuate(): int32 (B, 4), every junction's (phase, stage, timer, idle)
        self.lights: Optional[torch.Tensor] = None           # ... int32 (B,), the lights of the last step, 2 bits per signal group
        self.calls: Optional[torch.Tensor] = None            # ... int32 (B,), bit g = group g was called in the last step
        self._actuation = None
        self.advised: Optional[torch.Tensor] = None          # advise_speed(): float64 (P,), the speed advised in the last step, 0 = none
        self._advice = None
        self.share: Optional[torch.Tensor] = None            # share_plans(): int32 (P,), nonzero = the agent shares its plan
        self.shared_frames: Optional[torch.Tensor] = None    # ... int32 (P,), frames of the agent's row taken from its plan in the last step
        self._intent = None
        self.granted: Optional[torch.Tensor] = None          # reserve(): int32 (P,), 1 = the agent holds a reservation of the crossing
        self.since: Optional[torch.Tensor] = None            # ... int32 (P,), the junction clock at the agent's first request, -1 = none
        self.junction_clock: Optional[torch.Tensor] = None   # ... int32 (B,), every junction's clock
        self.occupied: Optional[torch.Tensor] = None         # ... int32 (B,), the movements that held the crossing in the last step
        self.queued: Optional[torch.Tensor] = None           # ... int32 (B,), the requesters denied in the last step
        self._reservation = None
        self.leader: Optional[torch.Tensor] = None           # follow(): int32 (P,), the pool row of the agent's leader in the last step, -1 = none
        self.gap: Optional[torch.Tensor] = None              # ... float64 (P,), the distance to it along the agent's path, -1 = none
        self.follow_cap: Optional[torch.Tensor] = None       # ... float64 (P,), the safe speed behind it, 0 = none
        self._following = None                               # (not a stage of _lib.STAGES: it is set on the context, _claim_context)
        self.partner: Optional[torch.Tensor] = None          # watch_safety(): int32 (P,), the pool row nearest to the agent in the last step, -1 = none
        self.near_clearance: Optional[torch.Tensor] = None   # ... float64 (P,), its clearance, +inf = none
        self.ttc_row: Optional[torch.Tensor] = None          # ... int32 (P,), the pool row of the first predicted contact, -1 = none
        self.ttc_frame: Optional[torch.Tensor] = None        # ... int32 (P,), its frame: (frame + 1) ip.dt seconds ahead, -1 = none
        self.n_events: Optional[torch.Tensor] = None         # ... int32 (P,), encounters opened so far, stored or not
        self._safety = None                                  # (set on the context too)
        self.sight: Optional[torch.Tensor] = None            # occlude(): int64 (P,), the bits of the uint64 word: bit j = the row at window offset j is seen
        self.n_seen: Optional[torch.Tensor] = None           # ... int32 (P,), rows seen in the last step
        self.n_hidden: Optional[torch.Tensor] = None         # ... int32 (P,), candidates not seen in the last step
        self._sight = None                                   # (set on the context too)
        self._sight_tabs = None                              # ... the device tables the struct names: hp, hp_off, box, set_off, set_of, heard or None
        self.boxed: Optional[torch.Tensor] = None            # keep_clear(): int32 (P,), 1 = the agent was kept at its line in the last step
        self.box_waited: Optional[torch.Tensor] = None       # ... int32 (P,), 1 = the agent stood at its line (held or boxed) in the last step
        self.box_occupied: Optional[torch.Tensor] = None     # ... int32 (B,), the movements inside the crossing in the last step
        self.n_boxed: Optional[torch.Tensor] = None          # ... int32 (B,), the agents boxed in the last step
        self._keepclear = None                               # (set on the context too)
        self._keepclear_tabs = None                          # ... the device tables the struct names: path_move, path_exit, conflict
        self.yielding: Optional[torch.Tensor] = None         # priority_road(): int32 (P,), 1 = the agent was kept at its line in the last step
        self.yield_waited: Optional[torch.Tensor] = None     # ... int32 (P,), the same word as the stage's memory (in-out)
        self.blocker: Optional[torch.Tensor] = None          # ... int32 (P,), the agent whose arrival is the lag, -1 = none
        self.lag: Optional[torch.Tensor] = None              # ... float64 (P,), seconds to the first conflicting car of smaller rank, +inf = none
        self.crossing: Optional[torch.Tensor] = None         # ... int32 (B,), the movements inside the crossing in the last step
        self.n_yielding: Optional[torch.Tensor] = None       # ... int32 (B,), the agents yielding in the last step
        self._priority = None                                # (set on the context too)
        self._priority_tabs = None                           # ... the device tables the struct names: path_stop, path_move, path_exit, conflict, rank, gap
        self.stopping: Optional[torch.Tensor] = None         # stop_signs(): int32 (P,), 1 = the agent was held at its line in the last step
        self.stopped_at: Optional[torch.Tensor] = None       # ... int32 (P,), the junction clock at which the agent completed its stop, -1 = not yet
        self.released: Optional[torch.Tensor] = None         # ... int32 (P,), 1 = the agent has been released into the crossing (or is inside)
        self.sign_lag: Optional[torch.Tensor] = None         # ... float64 (P,), seconds to the first conflicting unsigned car, +inf = none
        self.sign_blocker: Optional[torch.Tensor] = None     # ... int32 (P,), the agent whose arrival is the lag, -1 = none
        self.sign_clock: Optional[torch.Tensor] = None       # ... int32 (B,), every junction's clock
        self.ran_sign: Optional[torch.Tensor] = None         # ... int32 (B,), the cars that entered a signed movement unreleased, so far
        self.sign_occupied: Optional[torch.Tensor] = None    # ... int32 (B,), the movements inside the crossing or released into it in the last step
        self.n_waiting: Optional[torch.Tensor] = None        # ... int32 (B,), the agents held in the last step
        self._stopsign = None                                # (set on the context too)
        self._stopsign_tabs = None                           # ... the device tables the struct names
        self.firm: Optional[torch.Tensor] = None             # hold_firmly(): int32 (P,), 0 or the stop index e of an agent held at its line in the last step
        self.overran: Optional[torch.Tensor] = None          # ... int32 (P,), the steps in which the agent was held while physically beyond its line
        self.brake_cap: Optional[torch.Tensor] = None        # ... float64 (P,), the braking profile at the head of the window, 0.0 = not held at a line
        self._braking = None                                 # (set on the context too)
        self._win_len = None                                 # ... step_staged(): int32 (P,), the lengths the window stage is handed in place of path_len

    def attach_log(self, capacity: int, goal_dis: Optional[float] = None, stop_speed: Optional[float] = None,
                   max_bytes: Optional[int] = RUN_LOG_MAX_BYTES) -> RunLog:
        """Record every further step on the device (RunLog): `capacity` rows per agent, 96 bytes each -- 4096 x 8 agents x 100 steps are
        315 MB --, + 24 bytes per agent; capacity = 0 keeps the per-agent outcomes only.  A log larger than max_bytes is refused
        (max_bytes = None: no limit).  goal_dis / stop_speed default to GOAL_DIS / STOP_SPEED of lib/mpc.py (1.5 m, 0.1389 m/s).
        Costs one more launch per step; detach_log() restores the launches of a batch without a log."""
        from .lib import mpc as _mpc
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError('run log: negative capacity')
        need = capacity * self.P * _lib.RUN_LOG_ROW_BYTES + self.P * _lib.RUN_LOG_AGENT_BYTES
        if max_bytes is not None and need > max_bytes:
            raise ValueError('run log: %d rows x %d agents x %d bytes = %.1f MB exceed the limit of %.1f MB; pass a smaller capacity '
                             '(0 = outcomes only) or a larger max_bytes (None = no limit)'
                             % (capacity, self.P, _lib.RUN_LOG_ROW_BYTES, need / 1e6, max_bytes / 1e6))
        goal_dis, stop_speed = _mpc.GOAL_DIS if goal_dis is None else goal_dis, _mpc.STOP_SPEED if stop_speed is None else stop_speed
        if self._retire is not None and (float(goal_dis), float(stop_speed)) != (self._retire.goal_dis, self._retire.stop_speed):
            raise MpcxError('run log: goal_dis / stop_speed (%r, %r) differ from those agents are retired with (%r, %r): goal_step and '
                            'steps_driven would disagree' % (goal_dis, stop_speed, self._retire.goal_dis, self._retire.stop_speed))
        self.log = RunLog(self, capacity, goal_dis, stop_speed)
        self._desc = None
        return self.log

    def detach_log(self) -> Optional[RunLog]:
        """stop recording (the RunLog keeps what it holds); the batch enqueues exactly the launches of one that never had a log"""
        log, self.log = self.log, None
        self._desc = None
        return log

    def _stage_structs(self) -> dict:
        """the struct of every stage of _lib.STAGES as the batch stands, None = off: the keywords of Context.closed_loop_run"""
        return {k: (None if self.log is None else self.log.c) if k == 'log' else getattr(self, '_' + k) for k in _lib.STAGE_KEYS}

    def _off(self, *stages):
        """switch the named stages off, and with each the stages that live on it (_lib.stage_dependents); drops the cached descriptor"""
        entry = self._precedence is not None and self._precedence.mode == _lib.PRECEDENCE_ENTRY
        for k in stages:
            if k in ('sight', 'keepclear', 'priority', 'stopsign'):     # (attached to the context, no row of _lib.STAGES: nothing lives on it)
                setattr(self, '_' + k, None)
                continue
            off = {k} | _lib.stage_dependents(k, entry)
            if off & {'retire', 'scene'}:   # line of sight lives on the scene
                self._sight = None
            if 'signals' in off:            # keep clear lives on the signals
                self._keepclear = None
            for d in off:
                setattr(self, '_' + d, None)
        self._desc = None

    def _goal_now(self, goal_dis: float, stop_speed: float) -> np.ndarray:
        """mpc.is_goal (lib/mpc.py:310-326) on the host for every agent as the batch stands: the test at the top of the reference's next
        loop iteration (RunLog.reset() makes the same one for goal_step = 0).  Before the first step only a path of fewer than 5 points
        passes it.  Synchronises."""
        self.ctx.synchronize()
        path = self.path.cpu().numpy()
        off, ln = self.path_off.cpu().numpy().astype(np.int64), self.path_len.cpu().numpy().astype(np.int64)
        cut = self.inter['cut_len'].cpu().numpy().astype(np.int64)
        cut = ln if self.stop_mode == 'speed' else np.where(cut > 0, cut, ln)       # len(self.cx)
        goal, st = path[off + ln - 1], self.state.cpu().numpy()
        return ((np.hypot(st[:, 0] - goal[:, 0], st[:, 1] - goal[:, 1]) <= goal_dis) & (np.abs(self.target_ind.cpu().numpy() - cut) < 5) &
                (np.abs(st[:, 2]) <= stop_speed))

    def retire_at_goal(self, goal_dis: Optional[float] = None, stop_speed: Optional[float] = None, leave_scene: bool = False):
        """End every agent's episode where the reference's loop ends (`if mpc.is_goal(state): break`, scenarios/mpc_intersection.py:92-93):
        the step in which an agent arrives sets done[q] = 1, and from the next step on the agent keeps its state, has applied = (0, 0) -- to
        the others it is a parked car --, is not solved (its sol / pre / inter rows, target_ind and traj_idx stay as its last driven step
        left them), gets no further row in the run log and is not counted in closed_loop_stats().  Its pool row is still packed every step:
        arrived cars stay in the scene.  Costs one more launch per step (mpcx_closed_loop_run_retire); keep_driving() switches it off.
        goal_dis / stop_speed default to GOAL_DIS / STOP_SPEED of lib/mpc.py, as attach_log's do; with a log attached they must be the log's,
        so that goal_step == steps_driven for every retired agent (both count from the call that created them: attach the log and switch
        retirement on at the same step).  Allocates `done` and `steps_driven` (device, int32, P), makes the goal test before the first step
        on the host, and drops the cached descriptor.  Needs run(): step_staged(), a callable exchange and lin_passes > 1 are refused.
        leave_scene=True is DEPARTURE (mpcx_closed_loop_run_scene): the arrival also sets the agent's word of `absent` (device, int32, one
        per pool row, allocated here; the rows of agents that pass the goal test now are set at once), and from the next step on that row is
        in nobody's obstacle list and nobody's clearance, and is not predicted.  The agent's own buffers, done, steps_driven, the log and
        the statistics are those of retirement alone.  Rows may also be preset by the caller (`sim.absent[row] = 1` before run()), e.g. a
        scripted actor's row (`sim.actor_row`), to hide that vehicle from everybody.  An agent whose own row (`sim.obs_skip[q]`) is absent
        but which still drives is a ghost: it sees the others, they do not see it.  Refused with exchange='rccl' (a remote rank's mask
        would have to travel with the all-gather)."""
        if leave_scene and (self.exchange == 'rccl' or self.obs_local is not None):
            raise MpcxError('retire_at_goal(leave_scene=True) in the agent-sharded layout: a remote rank\'s absent mask would have to travel '
                            'with the all-gather (MPCX_E_INVALID); leave_scene=False, or shard by instances')
        from .lib import mpc as _mpc
        goal_dis = float(_mpc.GOAL_DIS if goal_dis is None else goal_dis)
        stop_speed = float(_mpc.STOP_SPEED if stop_speed is None else stop_speed)
        if not (np.isfinite(goal_dis) and np.isfinite(stop_speed) and goal_dis >= 0 and stop_speed >= 0):
            raise MpcxError('retire_at_goal: goal_dis = %r, stop_speed = %r must be finite and >= 0 (MPCX_E_INVALID)' % (goal_dis, stop_speed))
        if self.log is not None and (goal_dis, stop_speed) != (self.log.goal_dis, self.log.stop_speed):
            raise MpcxError('retire_at_goal: goal_dis / stop_speed (%r, %r) differ from the attached run log\'s (%r, %r): goal_step and '
                            'steps_driven would disagree' % (goal_dis, stop_speed, self.log.goal_dis, self.log.stop_speed))
        there = self._goal_now(goal_dis, stop_speed)
        self.done = self.ctx.i32(there.astype(np.int32))
        self.steps_driven = torch.zeros(self.P, dtype=torch.int32, device=self.ctx.device)
        if there.any():
            self.applied[torch.as_tensor(there, device=self.ctx.device)] = 0.0
        self._retire = _lib.RetireC(self.done.data_ptr(), self.steps_driven.data_ptr(), goal_dis, stop_speed)
        self.absent = None
        self._off('scene')                  # (... and what lives on it: enter_on_schedule(), give_way() after this call)
        if leave_scene:
            rows = int(self.obs6.shape[0])
            self.absent = torch.zeros(rows, dtype=torch.int32, device=self.ctx.device)
            if there.any():
                self.absent[self.obs_skip.long()[torch.as_tensor(there, device=self.ctx.device)]] = 1
            self._scene = _lib.SceneC(self.absent.data_ptr(), rows, 0)
        self.ctx.synchronize()

    def keep_driving(self):
        """switch retirement off: the batch enqueues exactly the launches of one that never had it.  Agents already retired stay where
        they are and are driven again from there; `done` and `steps_driven` keep what they hold until the next retire_at_goal().  The
        scene goes with it: every car, departed or hidden, is visible again from the next step on (`absent` keeps what it holds and is
        no longer read).  Admission goes with it too: agents still waiting are driven from where they stand, from the next step on -- and
        respawn with admission: no slot is reset any more"""
        self._off('retire')

    def enter_on_schedule(self, wait, gap: float = 0.0):
        """ADMISSION (mpcx_closed_loop_run_admit), the counterpart of departure: agent q with wait[q] >= 0 is taken out of the scene now
        (done[q] = 1 and its own row absent: not solved, not logged, not counted, not seen; its buffers stay as they were allocated) and
        asks to enter in the step in which its count-down ends -- wait[q] = 0: the very next step.  It is let in, on the device and as
        the first thing of a step, once its start pose has clearance >= gap [m] (the run log's clearance) to every vehicle present and to
        every lower-numbered agent that is due in the same step; until then it asks again every step.  From its admission on it is an
        agent like any other, and the step of its admission is the first step it drives.
        wait: integer array (B, A) or (P,), -1 = present from the start.  Needs retire_at_goal(leave_scene=True) first.  Allocates `wait`,
        `entered_step` (-1 until the agent is in; 0 for agents present from the start) and `clock` (steps completed since this call) on
        the device and drops the cached descriptor.  enter_now() switches admission off; keep_driving() does so together with retirement."""
        if self._scene is None:
            raise MpcxError('enter_on_schedule: admission needs a scene (MPCX_E_INVALID): retire_at_goal(leave_scene=True) first -- a waiting '
                            'agent is a retired one whose own row is absent')
        gap = float(gap)
        if not (np.isfinite(gap) and gap >= 0.0):
            raise MpcxError('enter_on_schedule: gap = %r must be finite and >= 0 (MPCX_E_INVALID)' % (gap,))
        w = np.asarray(wait)
        if not np.issubdtype(w.dtype, np.integer) or w.size != self.P or w.shape not in ((self.B, self.A), (self.P,)):
            raise ValueError('enter_on_schedule: wait must be an integer array of shape (B, A) = %s or (P,)' % ((self.B, self.A),))
        w = w.reshape(-1).astype(np.int64)
        if (w < -1).any() or (w > np.iinfo(np.int32).max).any():
            raise ValueError('enter_on_schedule: wait holds -1 (present from the start) or a number of steps >= 0')
        self.ctx.synchronize()
        sched = torch.as_tensor(w >= 0, device=self.ctx.device)
        self.done[sched] = 1
        self.absent[self.obs_skip.long()[sched]] = 1
        self.wait = self.ctx.i32(w)
        self.entered_step = self.ctx.i32(np.where(w >= 0, -1, 0))
        self.clock = torch.zeros(1, dtype=torch.int32, device=self.ctx.device)
        self.scheduled_step = np.maximum(w, 0)
        self._admit = _lib.AdmitC(self.wait.data_ptr(), self.entered_step.data_ptr(), self.clock.data_ptr(), 0, gap)
        self._off('respawn')                # (a new schedule and a new clock: respawn_on_schedule() sets both up itself)
        self.ctx.synchronize()

    def enter_now(self):
        """switch admission off and nothing else: the batch enqueues exactly the launches of one that never had it.  Agents still waiting
        stay outside the scene (retired, their rows absent); `wait`, `entered_step` and `clock` keep what they hold.  Respawn lives on admission
        and is switched off with it, and routing with respawn"""
        self._off('admit')                  # (the order of entry is admission's: give_way(order=<array>) keeps a fixed order)

    def respawn_on_schedule(self, due, gap: float = 0.0, route=None, start_index=None):
        """RESPAWN (mpcx_closed_loop_run_respawn): every slot (agent index q) serves a stream of G vehicles, all on the slot's route from the
        slot's start pose -- `state` and `traj_idx` of the batch as it stands.  due[q][g] is the step (counted from this call) at which vehicle
        g of slot q asks to enter.  When a slot's vehicle arrives, the last launch of that step writes the finished episode into the episode
        table (episodes()), puts the slot's per-agent state back to the first step of a fresh batch and hands it to the admission gate with
        wait = max(0, due of the next vehicle - next step); after its G-th vehicle the slot stays departed.  All on the device, under plain
        enqueue and graph replay alike; costs one more launch per step.
        due: integer array (B, A, G) or (P, G), values >= 0.  Needs retire_at_goal(leave_scene=True) first.  Calls
        enter_on_schedule(wait=due[..., 0], gap): every FIRST vehicle goes through the gate too -- two slots that share a start pose must never
        be present together at step 0 (in cut mode both cars would stand inside each other and yield for ever).  Allocates `served` and the
        episode table, and drops the cached descriptor.  With a run log attached a slot's rows are its vehicles' rows one after the other:
        size the log for the sum.  stop_respawning() switches respawn off alone; enter_now() and keep_driving() switch it off with what it
        lives on.
        route: ROUTES (mpcx_closed_loop_run_routes) -- an integer array of due's shape, (B, A, G) or (P, G), indexing the batch's `routes`:
        vehicle g of slot q drives route[q][g], and the reset that hands the slot to the gate also writes the slot's `path_off` / `path_len`
        (same number of launches as respawn alone; nothing in the hot kernels changes).  start_index: same shape, the path index every vehicle
        starts from; default the slot's current `traj_idx`, which must lie inside every route the slot takes (else ValueError).  A vehicle's
        start pose is the route point at its start index and its start speed the slot's current one; `pose_offset` is NOT re-applied: every
        routed vehicle, the first included, starts exactly on its route.  Everything is validated in numpy before anything is uploaded or
        changed; vehicle 0's route, pose and index are written into `path_off`, `path_len`, `state`, `traj_idx` and `target_ind` here, before
        the first vehicle goes through the gate.  The finished episodes then carry their route (episode_routes(), movement_summary()).
        route=None: exactly the batch described above -- a slot keeps its route and start pose."""
        if self._scene is None:
            raise MpcxError('respawn_on_schedule: respawn needs admission, which needs a scene (MPCX_E_INVALID): retire_at_goal(leave_scene=True) first')
        d = np.asarray(due)
        if not np.issubdtype(d.dtype, np.integer) or d.ndim not in (2, 3) or d.shape[:-1] not in ((self.B, self.A), (self.P,)) or d.shape[-1] < 1:
            raise ValueError('respawn_on_schedule: due must be an integer array of shape (B, A, G) = %s or (P, G), G >= 1' % ((self.B, self.A, 'G'),))
        d = d.reshape(self.P, -1).astype(np.int64)
        if (d < 0).any() or (d > np.iinfo(np.int32).max).any():
            raise ValueError('respawn_on_schedule: due holds step indices >= 0')
        G = int(d.shape[1])
        routed = None
        if route is None:
            if start_index is not None:
                raise ValueError('respawn_on_schedule: start_index is the start index per vehicle of a routed run: pass route too')
        else:
            routed = self._routed_tables(route, start_index, np.asarray(due).shape, G)
            self.ctx.synchronize()
            r0, s0 = routed['route'][:, 0], routed['start_idx'][:, 0]
            self.path_off.copy_(self.ctx.i32(self._route_offs[r0]))             # (in place: the descriptor and the routes struct name these words)
            self.path_len.copy_(self.ctx.i32(np.diff(self._route_offs)[r0]))
            self.state.copy_(self.ctx.f64(routed['start_state'][:, 0]))
            self.traj_idx.copy_(self.ctx.i32(s0)); self.target_ind.copy_(self.ctx.i32(s0))
        self.enter_on_schedule(d[:, 0], gap)
        dev = self.ctx.device
        self.start_state, self.start_idx = self.state.clone(), self.traj_idx.clone()
        self.due = self.ctx.i32(d)
        self.served = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self.ep_i32 = torch.zeros((self.P, G, 8), dtype=torch.int32, device=dev)
        self.ep_f64 = torch.zeros((self.P, G, 2), dtype=torch.float64, device=dev)
        self._respawn = _lib.RespawnC(G, 0, self.start_state.data_ptr(), self.start_idx.data_ptr(), self.due.data_ptr(), self.served.data_ptr(),
                                      self.ep_i32.data_ptr(), self.ep_f64.data_ptr())
        self.route_of = self.route_start_state = self.route_start_idx = self.route_off = self.route_len = None
        if routed is not None:
            self.route_of, self.route_start_idx = self.ctx.i32(routed['route']), self.ctx.i32(routed['start_idx'])
            self.route_start_state = self.ctx.f64(routed['start_state'])
            self.route_off, self.route_len = self.ctx.i32(self._route_offs[:-1]), self.ctx.i32(np.diff(self._route_offs))
            self._routes = _lib.RoutesC(len(self._route_offs) - 1, 0, self.route_off.data_ptr(), self.route_len.data_ptr(), self.route_of.data_ptr(),
                                        self.route_start_state.data_ptr(), self.route_start_idx.data_ptr(), self.path_off.data_ptr(),
                                        self.path_len.data_ptr())
        self._desc = None
        self.ctx.synchronize()

    def _routed_tables(self, route, start_index, due_shape, G: int) -> dict:
        """respawn_on_schedule(route=...): the per-vehicle tables on the host -- route (P, G), start_idx (P, G), start_state (P, G, 4) --,
        everything checked in numpy (ValueError); nothing is uploaded or changed"""
        offs, lens = self._route_offs, np.diff(self._route_offs)
        R = len(lens)
        r = np.asarray(route)
        if not np.issubdtype(r.dtype, np.integer) or r.shape != tuple(due_shape):
            raise ValueError('respawn_on_schedule: route must be an integer array of due\'s shape %s, got %s' % (tuple(due_shape), r.shape))
        r = r.reshape(self.P, G).astype(np.int64)
        if (r < 0).any() or (r >= R).any():
            raise ValueError('respawn_on_schedule: route indexes the batch\'s %d routes' % R)
        if start_index is None:
            s = np.repeat(self.traj_idx.cpu().numpy().astype(np.int64)[:, None], G, axis=1)
        else:
            s = np.asarray(start_index)
            if not np.issubdtype(s.dtype, np.integer) or s.shape != tuple(due_shape):
                raise ValueError('respawn_on_schedule: start_index must be an integer array of due\'s shape %s, got %s' % (tuple(due_shape), s.shape))
            s = s.reshape(self.P, G).astype(np.int64)
        bad = (s < 0) | (s >= lens[r])
        if bad.any():
            q, g = (int(v[0]) for v in np.nonzero(bad))
            raise ValueError('respawn_on_schedule: vehicle %d of slot %d starts at index %d of route %d, which has %d points%s'
                             % (g, q, s[q, g], r[q, g], lens[r[q, g]], '' if start_index is not None else
                                ' (the default start index is the slot\'s current traj_idx: it must lie inside every route the slot takes)'))
        pts = self._route_table[offs[r] + s]
        st = np.zeros((self.P, G, 4))
        st[..., 0], st[..., 1], st[..., 3] = pts[..., 0], pts[..., 1], pts[..., 2]
        st[..., 2] = self.state.cpu().numpy()[:, 2][:, None]
        return dict(route=r, start_idx=s, start_state=st)

    def give_way(self, order='entry'):
        """RIGHT OF WAY (mpcx_closed_loop_run_precedence).  Without it every agent yields to every other agent -- the reference's rule for
        its one ego among scripted cars --, and cars that meet at the crossing wait for each other for ever.  With it there is one precedence
        word per pool row, `prec` (device, int32; a smaller word goes first), and an agent sees a present car whose word is LARGER than its
        own as a STANDING car at its present pose: still an obstacle where it is, no longer a claim on the road ahead of it.  Cars with a
        smaller or equal word are seen through their prediction, as ever (equal words: the mutual yield).  The run log's clearance and
        contact stay true clearance; the admission gate, retirement, respawn and routes do not change.
        order='entry': first come, first served (MPCX_PRECEDENCE_ENTRY; needs enter_on_schedule() or respawn_on_schedule() first): one more
        small launch per step writes entered_step * 64 + window offset into the word of every agent in the scene, so a vehicle that enters
        -- a respawned one too -- queues behind everybody already there, ties to the lower agent index.
        order=<integer array (B, A) or (P,)>: a fixed word per agent (MPCX_PRECEDENCE_FIXED); the loop never writes `prec`.
        The rows of scripted cars hold zero -- every agent with a word >= 0 sees them moving; write `sim.prec[sim.actor_row]` to change that.
        Needs retire_at_goal(leave_scene=True) first.  Allocates `prec` and `stand` and drops the cached descriptor.  yield_to_everyone()
        switches it off; keep_driving() and retire_at_goal() drop it with the scene, enter_now() drops order='entry' with admission."""
        if self._scene is None:
            raise MpcxError('give_way: right of way needs a scene (MPCX_E_INVALID): retire_at_goal(leave_scene=True) first')
        rows = int(self.obs6.shape[0])
        words = np.zeros(rows, dtype=np.int64)
        if isinstance(order, str):
            if order != 'entry':
                raise ValueError('give_way: order is \'entry\' or an integer array with one word per agent, got %r' % (order,))
            if self._admit is None:
                raise MpcxError('give_way(order=\'entry\'): the order of entry needs admission (MPCX_E_INVALID): enter_on_schedule() or '
                                'respawn_on_schedule() first')
            mode = _lib.PRECEDENCE_ENTRY
        else:
            w = np.asarray(order)
            if not np.issubdtype(w.dtype, np.integer) or w.size != self.P or w.shape not in ((self.B, self.A), (self.P,)):
                raise ValueError('give_way: order must be \'entry\' or an integer array of shape (B, A) = %s or (P,)' % ((self.B, self.A),))
            w = w.reshape(-1).astype(np.int64)
            if (w < np.iinfo(np.int32).min).any() or (w > np.iinfo(np.int32).max).any():
                raise ValueError('give_way: the precedence words are int32')
            self.ctx.synchronize()
            words[self.obs_skip.cpu().numpy().astype(np.int64)] = w
            mode = _lib.PRECEDENCE_FIXED
        self.prec = self.ctx.i32(words)
        self.stand = torch.zeros((rows, 4), dtype=torch.float64, device=self.ctx.device)
        self._precedence = _lib.PrecedenceC(self.prec.data_ptr(), self.stand.data_ptr(), rows, mode)
        self._desc = None
        self.ctx.synchronize()

    def yield_to_everyone(self):
        """switch right of way off and nothing else: the batch enqueues exactly the launches of one that never had it, and every agent
        yields to every other again (`prec` keeps what it holds and is no longer read)"""
        self._off('precedence')

    def _route_list(self) -> list:
        return [self._route_table[self._route_offs[k]:self._route_offs[k + 1]] for k in range(len(self._route_offs) - 1)]

    def _line_tables(self, who: str, tabs: tuple, default) -> tuple:
        """the per-path-point tables of signalise / actuate (stop, group) and reserve (stop, group, exit): the caller's, all of them or
        none -- then default(the batch's routes) --, one word per path point"""
        names = ('stop and group', 'both stop and group, or neither') if len(tabs) == 2 else ('stop, group and exit', 'stop, group and exit, or none of them')
        if any(t is None for t in tabs):
            if any(t is not None for t in tabs):
                raise ValueError('%s: give %s' % (who, names[1]))
            tabs = default(self._route_list())
        tabs = tuple(np.asarray(t) for t in tabs)
        n_points = int(self.path.shape[0])
        if any(t.shape != (n_points,) for t in tabs):
            raise ValueError('%s: %s hold one word per path point (%d)' % (who, names[0], n_points))
        return tabs

    def _per_instance(self, who: str, name: str, v) -> np.ndarray:
        """the controller (actuate) or manager (reserve) of every instance: an integer array (B,), default 0"""
        v = np.zeros(self.B, dtype=np.int64) if v is None else np.asarray(v)
        if not np.issubdtype(v.dtype, np.integer) or v.shape != (self.B,):
            raise ValueError('%s: %s is an integer array of shape (B,) = (%d,)' % (who, name, self.B))
        return v

    def _brake(self, brake: Optional[float]) -> float:
        return abs(float(self.params.max_decel)) if brake is None else float(brake)

    def _planless_signals(self, tabs: dict, brake: float, n_groups: int):
        """the signals struct of actuate / reserve: the stop lines and the hold, the lights come from the junction's own stage"""
        self._signal_tabs = tabs
        self._signals = _lib.SignalsC(tabs['path_stop'].data_ptr(), tabs['path_group'].data_ptr(), None, None, None, None, None,
                                      self.held.data_ptr(), brake, int(self.path.shape[0]), 0, n_groups, 0)

    def signalise(self, plans, plan_of=None, stop=None, group=None, offset=None, brake: Optional[float] = None):
        """TRAFFIC SIGNALS (mpcx_closed_loop_run_signals).  One more small launch behind the conflict search holds an agent at its stop
        line while its light is red -- or amber, if it can still stop with `brake` or was held already --: the agent's path is cut on the point
        before the line (speed mode: its stop index is lowered to the line), exactly what the conflict search does in front of a conflict, so
        every later stage does the right thing; a conflict cut in front of the line is kept.
        plans: one plan or a sequence of plans, each dict(cycle, amber, green) with green of shape (n_groups, 2) = (green_from, green_len)
        per signal group, in steps (two_phase_plan() builds one); plan_of: the plan of every instance (B,) or agent (B, A) / (P,), default
        plan 0 -- a sweep of timings runs as one batch.  stop, group: the per-path-point tables (default: stop_lines() of the batch's
        routes).  offset: the initial signal clock per instance (B,) or agent (B, A) / (P,), default 0.  brake: default abs(MAX_DECEL) of the
        batch's parameters.
        Allocates `tick`, `held` (zero) and the tables and drops the cached descriptor.  Needs none of the other options and works with all
        of them; unsignalise() switches it off."""
        if isinstance(plans, dict):
            plans = [plans]
        plans = list(plans)
        if not plans:
            raise ValueError('signalise: at least one plan')
        green = [np.asarray(pl['green'], dtype=np.int64) for pl in plans]
        if any(g.ndim != 2 or g.shape != green[0].shape or g.shape[1] != 2 for g in green):
            raise ValueError('signalise: every plan\'s green has shape (n_groups, 2), the same n_groups in all plans')
        n_groups = int(green[0].shape[0])
        if not 1 <= n_groups <= _lib.SIGNAL_GROUPS_MAX:
            raise ValueError('signalise: %d signal groups, 1 .. %d' % (n_groups, _lib.SIGNAL_GROUPS_MAX))
        stop, group = self._line_tables('signalise', (stop, group), stop_lines)

        def per_agent(v, name, default):
            if v is None:
                return np.full(self.P, default, dtype=np.int64)
            v = np.asarray(v)
            if not np.issubdtype(v.dtype, np.integer) or v.shape not in ((self.B,), (self.B, self.A), (self.P,)):
                raise ValueError('signalise: %s is an integer array of shape (B,) = (%d,), (B, A) or (P,)' % (name, self.B))
            return (np.repeat(v, self.A) if v.shape == (self.B,) and self.B != self.P else v.reshape(-1)).astype(np.int64)
        plan_of, offset = per_agent(plan_of, 'plan_of', 0), per_agent(offset, 'offset', 0)
        brake = self._brake(brake)
        c = self.ctx
        tabs = dict(path_stop=c.i32(stop), path_group=c.i32(group), plan_cycle=c.i32(np.array([int(pl['cycle']) for pl in plans])),
                    plan_amber=c.i32(np.array([int(pl['amber']) for pl in plans])), plan_green=c.i32(np.stack(green)), plan_of=c.i32(plan_of))
        self.tick = c.i32(offset)
        self.held = torch.zeros(self.P, dtype=torch.int32, device=c.device)
        self._signal_tabs = tabs
        self._signals = _lib.SignalsC(tabs['path_stop'].data_ptr(), tabs['path_group'].data_ptr(), tabs['plan_cycle'].data_ptr(),
                                      tabs['plan_amber'].data_ptr(), tabs['plan_green'].data_ptr(), tabs['plan_of'].data_ptr(),
                                      self.tick.data_ptr(), self.held.data_ptr(), brake, len(stop), len(plans), n_groups, 0)
        self._off('actuation', 'reservation', 'priority', 'stopsign')   # (a junction is run by lights, by a manager, or by priority; a fixed plan replaces a controller or a junction manager as the source of the lights)
        c.synchronize()

    def advise_speed(self, v_min: float = 1.0, lead: int = 1, reach: float = 60.0, v_cruise: Optional[float] = None):
        """SIGNAL-AWARE APPROACH SPEED (mpcx_closed_loop_run_advised), for a batch in speed mode under signalise().  In speed mode a red
        light zeroes the speed reference from the stop line on while the position reference keeps pulling the car forward: it reaches the
        line at speed, brakes late and creeps over.  With advice an agent within `reach` metres of its line that would arrive on red at
        v_cruise (default: the batch's v_ref) has its speed reference capped at the speed with which it arrives `lead` steps after the
        light turns green, never below v_min: one more launch between the window stage and the QP.  The hold at the line is unchanged.
        Allocates `advised` (zero) and drops the cached descriptor; stop_advising() switches it off, as does unsignalise()."""
        if self.stop_mode != 'speed':
            raise ValueError('advise_speed: the batch runs with stop_mode=%r; advice caps the speed reference of stop_mode=\'speed\'' % self.stop_mode)
        if self._signals is None or self._actuation is not None:
            raise ValueError('advise_speed: needs signalise() -- a fixed plan to look ahead into (actuate() decides the lights step by step)')
        v_cruise = float(self.v_ref) if v_cruise is None else float(v_cruise)
        v_min, reach, lead = float(v_min), float(reach), int(lead)
        if not (np.isfinite([v_cruise, v_min, reach]).all() and v_cruise > 0 and v_min > 0 and reach > 0 and v_min <= v_cruise and lead >= 0):
            raise ValueError('advise_speed: 0 < v_min <= v_cruise, reach > 0, all finite, lead >= 0')
        self.advised = torch.zeros(self.P, dtype=torch.float64, device=self.ctx.device)
        self._advice = _lib.AdviceC(self.advised.data_ptr(), v_cruise, v_min, reach, lead, self.P)
        self._desc = None
        self.ctx.synchronize()

    def stop_advising(self):
        """switch the advice off and nothing else: the batch enqueues exactly the launches of one that never had it (`advised` keeps what
        it holds and is no longer written)"""
        self._off('advice')

    def follow(self, standstill: float = 6.0, time_gap: float = 1.0, brake: float = 3.0, v_min: float = 0.5, lateral: float = 1.5,
               heading: float = 0.8, reach: Optional[int] = None):
        """CAR FOLLOWING (mpcx_set_following), in both stop modes and beside every other stage.  The conflict search knows no leader: a
        queue, a platoon and two streams that merge have nothing that keeps them apart.  With following every agent looks `reach` path
        points ahead on its OWN path (default: 40 m of it) for the nearest vehicle of its pool window -- agents and scripted cars alike --
        that is within `lateral` metres of the path and heads along it within `heading` radians, and stops `standstill` metres (reference
        point to reference point: more than the 4.33 m at which the stock car's discs touch) plus `time_gap` seconds of its own speed
        behind it: the signals' hold at a line that moves.  In speed mode the stop point keeps `standstill` only and the time gap is in a
        cap on the speed reference, Gipps' safe speed for a deceleration `brake`, never below `v_min`.  One more launch in front of the
        window stage, in speed mode one more behind it.  Right of way is not consulted.  The defaults are those of the closed-loop runs of
        tests/test_follow_cpu.py.  Allocates `leader` (-1), `gap` (-1) and `follow_cap` (0) and drops the cached descriptor;
        stop_following() switches it off."""
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('follow: not in the agent-sharded layout (shard by instances)')
        reach = min(int(round(40.0 / self.dl)), _lib.MAX_REMAINING) if reach is None else int(reach)
        vals = [float(v) for v in (standstill, time_gap, brake, v_min, lateral, heading)]
        if not (np.isfinite(vals).all() and all(v > 0 for v in vals[:1] + vals[2:]) and vals[1] >= 0 and 1 <= reach <= _lib.MAX_REMAINING):
            raise ValueError('follow: standstill, brake, v_min, lateral, heading > 0, time_gap >= 0, all finite, reach in 1..%d points' % _lib.MAX_REMAINING)
        dev = self.ctx.device
        self.leader = torch.full((self.P,), -1, dtype=torch.int32, device=dev)
        self.gap = torch.full((self.P,), -1.0, dtype=torch.float64, device=dev)
        self.follow_cap = torch.zeros(self.P, dtype=torch.float64, device=dev)
        self._following = _lib.FollowingC(self.leader.data_ptr(), self.gap.data_ptr(), self.follow_cap.data_ptr(), *vals, reach, self.P, 0)
        self._desc = None
        self.ctx.synchronize()

    def stop_following(self):
        """switch following off and nothing else: the batch enqueues exactly the launches of one that never had it (`leader`, `gap` and
        `follow_cap` keep what they hold and are no longer written)"""
        self._following = None
        self._desc = None

    def hold_firmly(self, brake: float = 3.0, setback: float = 2.0):
        """FIRM HOLD (mpcx_set_braking), for stop_mode='speed'; in cut mode it only writes its words, the cut is hard already.  Every rule
        that stops a car at a line -- signalise(), actuate(), reserve(), keep_clear(), priority_road(), stop_signs() -- lowers the stop index to the line,
        and in speed mode that is soft: the window's position reference runs ahead at 10 km/h whatever the car does, and the path index of
        a standing car climbs a point a step until the hold sees it "on the line" and lets it go.  With the firm hold an agent whose hold
        word (`held`, `boxed`, `yielding`, `stopping` -- those of the stages that are on when a run is enqueued) is nonzero has its window built on
        the path up to a stop point ceil(setback / dl) points in front of its line, every entry of its speed reference capped at
        sqrt(2 brake d) with d the distance of that window point to the stop point, and its path index pinned to the stop point while it is
        physically behind the line (a half-plane test; a car that is beyond it is left to the hold, and counted in `overran`).  One small
        launch in front of the window stage and one behind it.  Needs a source of stop lines at run time; switching signals, keep clear or
        the priority road on or off afterwards leaves the firm hold on.  brake > 0; setback >= 2 dl.  Allocates `firm`, `overran` and
        `brake_cap` and drops the cached descriptor; hold_softly() switches it off."""
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('hold_firmly: not in the agent-sharded layout (shard by instances)')
        brake, setback = float(brake), float(setback)
        if not (np.isfinite(brake) and brake > 0 and np.isfinite(setback) and setback >= 2.0 * self.dl):
            raise ValueError('hold_firmly: brake > 0 and setback >= 2 dl = %g, both finite' % (2.0 * self.dl))
        if self._stopsign is not None and not self._stopsign.zone * self.dl > setback:
            raise ValueError('hold_firmly: setback = %g m is not inside the stop signs\' zone of %d points = %g m: a car standing on its firm stop '
                             'point could never stamp its stop' % (setback, self._stopsign.zone, self._stopsign.zone * self.dl))
        dev = self.ctx.device
        self.firm = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self.overran = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self.brake_cap = torch.zeros(self.P, dtype=torch.float64, device=dev)
        self._win_len = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self._braking = _lib.BrakingC(brake, setback, self.firm.data_ptr(), self.overran.data_ptr(), self.brake_cap.data_ptr())
        self._desc = None
        self.ctx.synchronize()

    def hold_softly(self):
        """switch the firm hold off and nothing else: the batch enqueues exactly the launches of one that never had it (`firm`, `overran`
        and `brake_cap` keep what they hold and are no longer written)"""
        self._braking = None
        self._desc = None

    @property
    def n_firm(self) -> int:
        """the number of agents the firm hold kept at a stop point in the last step (synchronises); 0 while off"""
        if self._braking is None:
            return 0
        self.ctx.synchronize()
        return int((self.firm != 0).sum().item())

    def _line_words(self):
        """the firm hold's view of the stages that are on now: (path_stop, held, boxed, yielding), None where there is none"""
        sig, pri, sgn = self._signals is not None, self._priority is not None, self._stopsign is not None
        stop = self._signal_tabs['path_stop'] if sig else self._priority_tabs['path_stop'] if pri else self._stopsign_tabs['path_stop'] if sgn else None
        # (the priority road and stop signs never run together: `stopping` travels where `yielding` does)
        return (stop, self.held if sig else None, self.boxed if self._keepclear is not None else None,
                self.yielding if pri else self.stopping if sgn else None)

    def watch_safety(self, near: float = 0.5, ttc: float = 2.0, capacity: int = 8):
        """THE NEAR-MISS LOG (mpcx_set_safety), beside every other stage and in both stop modes: one more launch directly behind the conflict
        search finds, for every driving agent, the vehicle of its pool window nearest to it (`partner`, `near_clearance`: the run log's
        clearance with a name to it) and the first frame of the prediction in which its discs touch another's (`ttc_row`, `ttc_frame`), and
        keeps a table of ENCOUNTERS per agent in device memory: an event opens when the clearance falls below `near` metres or a contact is
        predicted within `ttc` seconds (floor(ttc / ip.dt) frames), follows the same partner, and closes when neither holds; `capacity`
        events are stored per agent, further ones are counted.  The stage changes no decision and no other buffer.  near_misses() reads
        the events back, conflict_matrix() reduces them per pair of movements on the device.  Allocates the words (partner, ttc_row,
        ttc_frame, the open encounter = -1; near_clearance = +inf; the rest = 0) and drops the cached descriptor; stop_watching() switches
        it off.  Slots that respawn keep counting: an event carries its ticks and path_off."""
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('watch_safety: not in the agent-sharded layout (shard by instances)')
        if self.obs_skip is None:
            raise ValueError('watch_safety: the batch has no obs_skip (the agents\' own pool rows)')
        near, ttc, capacity = float(near), float(ttc), int(capacity)
        if not (np.isfinite(near) and near >= 0 and np.isfinite(ttc) and ttc >= 0 and capacity >= 0):
            raise ValueError('watch_safety: near >= 0, ttc >= 0, both finite, capacity >= 0')
        frames = min(int(np.floor(ttc / float(self.ip.dt))), int(self.ip.pred_steps))
        dev, P, rows = self.ctx.device, self.P, int(self.obs6.shape[0])
        owner = np.full(rows, -1, np.int32)
        own = self.obs_skip.cpu().numpy()
        ok = (own >= 0) & (own < rows)
        owner[own[ok]] = np.arange(P, dtype=np.int32)[ok]
        self._row_agent = self.ctx.i32(owner)
        full = lambda v, dt: torch.full((P,), v, dtype=dt, device=dev)
        self.partner, self.ttc_row, self.ttc_frame, self._enc_row = (full(-1, torch.int32) for _ in range(4))
        self.near_clearance = full(float('inf'), torch.float64)
        self._safety_tick, self.n_events = full(0, torch.int32), full(0, torch.int32)
        self._ev_i32 = torch.zeros((P, capacity, 8), dtype=torch.int32, device=dev)
        self._ev_f64 = torch.zeros((P, capacity, 2), dtype=torch.float64, device=dev)
        self._safety = _lib.SafetyC(self.partner.data_ptr(), self.near_clearance.data_ptr(), self.ttc_row.data_ptr(), self.ttc_frame.data_ptr(),
                                    self._safety_tick.data_ptr(), self._enc_row.data_ptr(), self.n_events.data_ptr(),
                                    self._ev_i32.data_ptr() if capacity else None, self._ev_f64.data_ptr() if capacity else None,
                                    self._row_agent.data_ptr(), near, frames, capacity, P, rows, 0)
        self._desc = None
        self.ctx.synchronize()

    def stop_watching(self):
        """switch the near-miss log off and nothing else: the batch enqueues exactly the launches of one that never had it (the words and
        the events keep what they hold and are no longer written)"""
        self._safety = None
        self._desc = None

    def near_misses(self) -> np.ndarray:
        """the stored events of the near-miss log, in agent order and, per agent, in the order they opened (synchronises): a structured
        array of NEAR_MISS_DTYPE -- agent, the words of _lib.SAFETY_I32 (open and last tick, the partner's pool row, row_agent: the agent that owns it
        or -1 for a scripted car, the two path offsets, traj_idx at opening, the smallest frame of a predicted contact or -1), min_clearance,
        v (the agent's speed at opening) and ttc = (ttc_frame + 1) ip.dt seconds, +inf without a predicted contact"""
        if self.n_events is None:
            raise MpcxError('near_misses(): watch_safety() has not been called')
        self.ctx.synchronize()
        wi, wf, n = self._ev_i32.cpu().numpy(), self._ev_f64.cpu().numpy(), self.n_events.cpu().numpy()
        q, e = np.nonzero(np.arange(wi.shape[1])[None, :] < n[:, None])
        out = np.zeros(len(q), NEAR_MISS_DTYPE)
        out['agent'] = q
        for k, name in enumerate(_lib.SAFETY_I32):
            out[name] = wi[q, e, k]
        out['min_clearance'], out['v'] = wf[q, e, 0], wf[q, e, 1]
        out['ttc'] = np.where(out['ttc_frame'] >= 0, (out['ttc_frame'] + 1.0) * float(self.ip.dt), np.inf)
        return out

    def conflict_matrix(self, routes=None) -> np.ndarray:
        """the conflict matrix of the near-miss log, reduced on the device (mpcx_safety_summary; one small launch; synchronises): a
        structured array (B, R + 1, R + 1) of CONFLICT_DTYPE -- per instance and pair (movement of the agent, movement of its partner),
        over the stored events: events, contacts (events whose minimum clearance is negative), predicted (events with a predicted
        contact), min_clearance and min_ttc in seconds (+inf: none).  routes: the route indices that are the classes, None = every
        route of the batch in order; class R -- the last row and column -- is "no route": a scripted car, or a route not listed."""
        if self.n_events is None:
            raise MpcxError('conflict_matrix(): watch_safety() has not been called')
        offs = self._route_offs[:-1] if routes is None else self._route_offs[:-1][np.asarray(routes, dtype=np.int64)]
        out_i, out_f = self.ctx.safety_summary(self.A, self.ctx.i32(offs.astype(np.int32)), float(self.ip.dt), self.n_events, self._ev_i32, self._ev_f64)
        self.ctx.synchronize()
        wi, wf = out_i.cpu().numpy(), out_f.cpu().numpy()
        out = np.zeros(wi.shape[:3], CONFLICT_DTYPE)
        for k, name in enumerate(_lib.SAFETY_SUMMARY_I64):
            out[name] = wi[..., k]
        for k, name in enumerate(_lib.SAFETY_SUMMARY_F64):
            out[name] = wf[..., k]
        return out

    def occlude(self, occluders, sensor_range: float = 60.0, shrink: float = 0.0, set_of=None, hear='shared'):
        """LINE OF SIGHT (mpcx_set_sight), beside every other stage: buildings hide cars from each other.  One more launch in front of the
        conflict search decides, per agent, which rows of its pool window it sees -- in range of `sensor_range` metres of its reference
        point and with no occluder across the segment from its reference point to the other's -- and the conflict search leaves the rows
        it does not see out of the agent's obstacle list, as it leaves out the departed ones.  Nothing else consults the word: the
        following stage, the near-miss log, the run log's clearance, the admission gate and a reservation manager read the physical scene.
        occluders: a list of `Obstacle`s (lib/obstacles.py: anything with to_convex()), or a list of such lists for a table of sets;
        set_of: the set of every instance, shape (B,), default 0 -- an empty list is an open junction, so a sweep of worlds is one batch.
        shrink >= 0 takes that much off every side of every occluder (to_convex(-shrink)): a car whose centre is just behind a corner is
        seen by its body.  hear: 'shared' -- the rows of the agents that share their plans (share_plans() first; taken as it stands now;
        nobody if the batch shares no plans) are seen wherever they are in range, a connected vehicle announces its pose --, None, or an
        int array over the pool rows.
        A world's own obstacle list (lib/scenario.py) is not a good occluder set as it stands: it contains the medians and the
        hidden=True wrong-way lanes, which are no buildings; corner_blocks() gives the four corner buildings of the stock four-way world.
        Needs retire_at_goal(leave_scene=True) first (the list of present rows is the scene's) and therefore run(): step_staged() has no
        retired mask.  Allocates `sight`, `n_seen`, `n_hidden` (zero) and the tables and drops the cached descriptor; see_everything()
        switches it off, keep_driving() and retire_at_goal() drop it with the scene."""
        if self._scene is None:
            raise MpcxError('occlude: line of sight needs a scene (MPCX_E_INVALID): retire_at_goal(leave_scene=True) first')
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('occlude: not in the agent-sharded layout (shard by instances)')
        sensor_range, shrink = float(sensor_range), float(shrink)
        if not (sensor_range > 0) or not (np.isfinite(shrink) and shrink >= 0):
            raise ValueError('occlude: sensor_range > 0 (inf allowed), shrink >= 0 and finite')
        occluders = list(occluders)
        sets = [list(s) for s in occluders] if occluders and all(isinstance(s, (list, tuple)) for s in occluders) else [occluders]
        hp, hp_off, box, set_off = occluder_table(sets, shrink)
        which = np.zeros(self.B, np.int64) if set_of is None else np.asarray(set_of)
        if which.shape != (self.B,) or which.dtype.kind not in 'iu' or (which < 0).any() or (which >= len(sets)).any():
            raise ValueError('occlude: set_of must be an integer array of shape (B,) = (%d,) with values in [0, %d)' % (self.B, len(sets)))
        dev, P, rows = self.ctx.device, self.P, int(self.obs6.shape[0])
        heard = None
        if isinstance(hear, str):
            if hear != 'shared':
                raise ValueError('occlude: hear is \'shared\', None or an int array over the %d pool rows' % rows)
            if self._intent is not None:
                self.ctx.synchronize()
                heard = np.zeros(rows, np.int32)
                own, flags = self.obs_skip.cpu().numpy().astype(np.int64), self.share.cpu().numpy()
                ok = (own >= 0) & (own < rows) & (flags != 0)
                heard[own[ok]] = 1
        elif hear is not None:
            heard = np.asarray(hear)
            if heard.shape != (rows,) or heard.dtype.kind not in 'biu':
                raise ValueError('occlude: hear must be an int array over the %d pool rows' % rows)
            heard = (heard != 0).astype(np.int32)
        f64 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
        self._sight_tabs = (f64(hp.reshape(-1)), self.ctx.i32(hp_off), f64(box.reshape(-1)), self.ctx.i32(set_off),
                            self.ctx.i32(np.repeat(which.astype(np.int32), self.A)), None if heard is None else self.ctx.i32(heard))
        t = self._sight_tabs
        self.sight = torch.zeros(P, dtype=torch.int64, device=dev)
        self.n_seen, self.n_hidden = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
        n_occ = len(hp_off) - 1
        self._sight = _lib.SightC(self.sight.data_ptr(), self.n_seen.data_ptr(), self.n_hidden.data_ptr(), t[0].data_ptr() if len(hp) else None,
                                  t[1].data_ptr(), t[2].data_ptr() if n_occ else None, t[3].data_ptr(), t[4].data_ptr(),
                                  None if t[5] is None else t[5].data_ptr(), sensor_range, n_occ, len(sets), P, rows, 0)
        self._desc = None
        self.ctx.synchronize()

    def see_everything(self):
        """switch line of sight off and nothing else: the batch enqueues exactly the launches of one that never had it (`sight`, `n_seen`
        and `n_hidden` keep what they hold and are no longer written)"""
        self._off('sight')

    def keep_clear(self, conflict=None, move=None, exit=None, detect: Optional[int] = None, phases=((0, 2), (1, 3))):
        """KEEP CLEAR (mpcx_set_keepclear), for a batch under signalise() or actuate(), in both stop modes.  The hold looks at the light
        and nothing else: under a two-phase plan the first car of a phase starts into a car of the phase before that is still crossing.
        With keep clear one more small launch behind the hold works out, per instance (a junction of A <= 64 agents), which movements are
        inside the crossing -- from the stop line to the exit point --, and an agent within `detect` path points of its line whose light
        lets it go, but whose movement conflicts with one that is inside, is held at its line by the cut the signal hold makes.  A car that
        stood at its line in the step before (held by the light or boxed) stays; a car that arrives at speed on green stays only if it can
        still stop with the signals' `brake`, else it is left to the conflict search, as on amber.  `held` stays the light's word.
        move, exit: the per-path-point tables, both or neither (default: movement_lines() of the batch's routes); conflict: one bit mask
        per movement, symmetric, without a diagonal (default: cross_phase_conflicts(movement_conflicts(...), phases) with the batch's disc
        model: only movements of arms that share no phase keep each other out, so a permissive turn is not blocked by the opposed arm);
        detect: default the whole approach (the largest stop-line index).
        Allocates `boxed`, `box_waited`, `box_occupied`, `n_boxed` (zero) and the tables and drops the cached descriptor;
        enter_on_green() switches it off, as does unsignalise() or reserve()."""
        if self._signals is None:
            raise ValueError('keep_clear: needs signalise() or actuate() -- the stage holds a car whose light lets it go')
        if self._reservation is not None:
            raise ValueError('keep_clear: the batch runs under reserve(), whose manager already keeps the crossing clear')
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('keep_clear: not in the agent-sharded layout (shard by instances)')
        if not 1 <= self.A <= _lib.KEEPCLEAR_PER_MAX:
            raise ValueError('keep_clear: a junction holds 1 .. %d agents, the batch has A = %d' % (_lib.KEEPCLEAR_PER_MAX, self.A))
        stop = self._signal_tabs['path_stop'].cpu().numpy()
        if move is None or exit is None:
            if move is not None or exit is not None:
                raise ValueError('keep_clear: give both move and exit, or neither')
            _, move, exit = movement_lines(self._route_list())
        move, exit = np.asarray(move), np.asarray(exit)
        n_points = int(self.path.shape[0])
        if move.shape != (n_points,) or exit.shape != (n_points,):
            raise ValueError('keep_clear: move and exit hold one word per path point (%d)' % n_points)
        if conflict is None:
            full, _ = movement_conflicts(self._route_list(), stop, exit, np.asarray(self.ip.circle_centers), float(self.ip.radius))
            conflict = cross_phase_conflicts(full, phases)
        conflict = np.asarray(conflict)
        if conflict.ndim != 1 or not 1 <= len(conflict) <= _lib.SIGNAL_GROUPS_MAX or not np.issubdtype(conflict.dtype, np.integer):
            raise ValueError('keep_clear: conflict holds one integer word per movement, 1 .. %d movements' % _lib.SIGNAL_GROUPS_MAX)
        detect = max(int(stop.max()) if len(stop) else 1, 1) if detect is None else int(detect)
        if not 1 <= detect <= int(np.iinfo(np.int32).max):
            raise ValueError('keep_clear: detect >= 1 path point, int32')
        c = self.ctx
        tabs = dict(path_move=c.i32(move), path_exit=c.i32(exit), conflict=c.i32(conflict))
        zeros = lambda n: torch.zeros(n, dtype=torch.int32, device=c.device)
        self.boxed, self.box_waited, self.box_occupied, self.n_boxed = zeros(self.P), zeros(self.P), zeros(self.B), zeros(self.B)
        self._keepclear_tabs = tabs
        self._keepclear = _lib.KeepClearC(tabs['path_move'].data_ptr(), tabs['path_exit'].data_ptr(), tabs['conflict'].data_ptr(),
                                          self.boxed.data_ptr(), self.box_waited.data_ptr(), self.box_occupied.data_ptr(),
                                          self.n_boxed.data_ptr(), detect, self.A, self.B, len(conflict), n_points, 0)
        c.set_keepclear(None)       # (a new table may sit where an old one sat: the context checks the next struct it is given afresh)
        self._desc = None
        c.synchronize()

    def enter_on_green(self):
        """switch keep clear off and nothing else: the batch enqueues exactly the launches of one that never had it (`boxed`, `box_waited`,
        `box_occupied` and `n_boxed` keep what they hold and are no longer written)"""
        self._off('keepclear')

    def priority_road(self, major=(0, 2), rank=None, gap=4.0, v_floor: float = 1.0, brake: Optional[float] = None, detect: Optional[int] = None,
                      stop=None, move=None, exit=None, conflict=None):
        """PRIORITY ROAD (mpcx_set_priority), for a batch without signals, in both stop modes: the junction most roads have, a major road
        crossed by a minor road under give-way signs.  One more small launch in the hold's place -- behind the conflict search, in front
        of the following stage -- works out, per instance (a junction of A <= 64 agents), for every agent within `detect` path points of
        its stop line the LAG: the least time `(s - traj_idx) dl / max(v, v_floor)` (0 inside the crossing) of a car of the junction whose
        movement conflicts with its own and has a smaller rank.  An agent whose lag is below its movement's critical `gap` (seconds) is
        held at its line by the cut the signal hold makes -- if it stood there in the step before, or if it can still stop with `brake`;
        else it is left to the conflict search, as on amber.  Equal ranks stay with the conflict search.
        major: the arms (0 .. 3) of the major road; rank: one non-negative integer per movement, a smaller rank goes first (default:
        priority_ranks(major)); gap: a scalar or one value per movement; stop, move, exit: the per-path-point tables, all of them or none
        (default: movement_lines() of the batch's routes); conflict: one bit mask per movement, symmetric, without a diagonal (default:
        the full movement_conflicts() table with the batch's disc model); detect: default the whole approach (the largest stop-line
        index); brake: default abs(MAX_DECEL) of the batch's parameters.
        Refused under signalise() / actuate() / reserve() -- a junction is run by lights, by a manager, or by priority; calling one of
        them later switches this stage off.  Allocates `yielding`, `yield_waited`, `blocker`, `lag`, `crossing`, `n_yielding` and the
        tables and drops the cached descriptor; all_roads_equal() switches it off."""
        if self._signals is not None or self._actuation is not None or self._reservation is not None:
            raise ValueError('priority_road: the batch runs under signalise(), actuate() or reserve() -- a junction is run by lights, by a '
                             'manager, or by priority')
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('priority_road: not in the agent-sharded layout (shard by instances)')
        if not 1 <= self.A <= _lib.PRIORITY_PER_MAX:
            raise ValueError('priority_road: a junction holds 1 .. %d agents, the batch has A = %d' % (_lib.PRIORITY_PER_MAX, self.A))
        if len({t is None for t in (stop, move, exit)}) > 1:
            raise ValueError('priority_road: give stop, move and exit, or none of them')
        stop, move, exit = self._line_tables('priority_road', (stop, move, exit), movement_lines)
        if conflict is None:
            conflict, _ = movement_conflicts(self._route_list(), stop, exit, np.asarray(self.ip.circle_centers), float(self.ip.radius))
        conflict = np.asarray(conflict)
        if conflict.ndim != 1 or not 1 <= len(conflict) <= _lib.SIGNAL_GROUPS_MAX or not np.issubdtype(conflict.dtype, np.integer):
            raise ValueError('priority_road: conflict holds one integer word per movement, 1 .. %d movements' % _lib.SIGNAL_GROUPS_MAX)
        n_moves = len(conflict)
        rank = np.asarray(priority_ranks(major) if rank is None else rank)
        if rank.shape != (n_moves,) or not np.issubdtype(rank.dtype, np.integer) or (rank < 0).any():
            raise ValueError('priority_road: rank holds one non-negative integer per movement (%d)' % n_moves)
        gap = np.broadcast_to(np.asarray(gap, dtype=np.float64), (n_moves,)) if np.ndim(gap) == 0 else np.asarray(gap, dtype=np.float64)
        if gap.shape != (n_moves,) or not np.isfinite(gap).all() or (gap < 0).any():
            raise ValueError('priority_road: gap is a finite, non-negative number of seconds, or one per movement (%d)' % n_moves)
        v_floor, brake = float(v_floor), self._brake(brake)
        if not (np.isfinite(v_floor) and v_floor > 0 and np.isfinite(brake) and brake > 0):
            raise ValueError('priority_road: v_floor and brake are finite and positive')
        detect = max(int(stop.max()) if len(stop) else 1, 1) if detect is None else int(detect)
        if not 1 <= detect <= int(np.iinfo(np.int32).max):
            raise ValueError('priority_road: detect >= 1 path point, int32')
        self._off('stopsign')       # (a junction is run by priority or by signs; behind the checks: a refused call changes nothing)
        c = self.ctx
        tabs = dict(path_stop=c.i32(stop), path_move=c.i32(move), path_exit=c.i32(exit), conflict=c.i32(conflict), rank=c.i32(rank),
                    gap=torch.as_tensor(np.ascontiguousarray(gap), dtype=torch.float64, device=c.device))
        zeros = lambda n: torch.zeros(n, dtype=torch.int32, device=c.device)
        self.yielding, self.yield_waited, self.crossing, self.n_yielding = zeros(self.P), zeros(self.P), zeros(self.B), zeros(self.B)
        self.blocker = torch.full((self.P,), -1, dtype=torch.int32, device=c.device)
        self.lag = torch.full((self.P,), float('inf'), dtype=torch.float64, device=c.device)
        self._priority_tabs = tabs
        self._priority = _lib.PriorityC(tabs['path_stop'].data_ptr(), tabs['path_move'].data_ptr(), tabs['path_exit'].data_ptr(),
                                        tabs['conflict'].data_ptr(), tabs['rank'].data_ptr(), tabs['gap'].data_ptr(),
                                        self.yield_waited.data_ptr(), self.yielding.data_ptr(), self.blocker.data_ptr(), self.lag.data_ptr(),
                                        self.crossing.data_ptr(), self.n_yielding.data_ptr(), v_floor, brake, detect, self.A, self.B, n_moves,
                                        int(self.path.shape[0]), 0)
        c.set_priority(None)        # (a new table may sit where an old one sat: the context checks the next struct it is given afresh)
        self._desc = None
        c.synchronize()

    def all_roads_equal(self):
        """switch the priority rule off and nothing else: the batch enqueues exactly the launches of one that never had it (`yielding`,
        `yield_waited`, `blocker`, `lag`, `crossing` and `n_yielding` keep what they hold and are no longer written)"""
        self._off('priority')

    def stop_signs(self, signed=None, gap=5.0, v_stop: float = 0.5, zone: Optional[int] = None, detect: Optional[int] = None,
                   brake: Optional[float] = None, v_floor: float = 1.0, patience: int = 0, stop=None, move=None, exit=None, conflict=None,
                   lane=None):
        """STOP SIGNS (mpcx_set_stopsign), for a batch without signals, in both stop modes: the all-way or two-way stop junction.  One more
        small launch in the hold's place -- behind the conflict search, in front of the following stage -- holds every car of a SIGNED
        movement at its stop line by the cut the signal hold makes until it has STOPPED there -- it stood at `v_stop` m/s or less within
        `zone` path points of its line; the junction clock of that step is its stamp, `stopped_at` -- and its turn has come: the stopped
        cars of a junction (an instance of A <= 64 agents) are released in the order of their stamps, the lower slot first among equals,
        each if its movement crosses none that is inside the crossing or released into it, no car of its own approach lane has just been
        denied in front of it, and no car of an unsigned movement that crosses its own reaches its line within the movement's critical
        `gap` (seconds; the lag is `(s - traj_idx) dl / max(v, v_floor)`).  A denied car that has waited `patience` steps since its stamp
        also blocks every later car that crosses it; a later car that crosses no earlier one may go.  A release is never revoked.  A car
        that can no longer stop with `brake` when it comes within `detect` points is left to the conflict search; `ran_sign` counts the
        cars that entered a signed movement without a release.
        signed: None = all-way, every movement carries a sign; else the arms (0 .. 3) that carry signs, the others being the through road
        (sign_table()), or one 0 / 1 word per movement.  gap: a scalar or one value per movement.  stop, move, exit: the per-path-point
        tables, all of them or none (default: movement_lines() of the batch's routes); conflict, lane: one bit mask per movement each,
        both or neither (default: movement_conflicts() with the batch's disc model).  zone: default ceil(4 / dl) points; detect: default
        the whole approach (the largest stop-line index, at least zone); brake: default abs(MAX_DECEL) of the batch's parameters.
        Refused under signalise() / actuate() / reserve() -- a junction is run by lights, by a manager, by priority, or by signs; calling
        one of them later switches this stage off, and it and priority_road() switch each other off.  With hold_firmly() on, zone dl must
        exceed the firm hold's setback: a car standing on its firm stop point could never stamp otherwise.  Allocates `stopping`,
        `stopped_at`, `released`, `sign_lag`, `sign_blocker`, `sign_clock`, `ran_sign`, `sign_occupied`, `n_waiting` and the tables and
        drops the cached descriptor; no_signs() switches it off."""
        if self._signals is not None or self._actuation is not None or self._reservation is not None:
            raise ValueError('stop_signs: the batch runs under signalise(), actuate() or reserve() -- a junction is run by lights, by a '
                             'manager, by priority, or by signs')
        if self.exchange == 'rccl' or callable(self.exchange):
            raise ValueError('stop_signs: not in the agent-sharded layout (shard by instances)')
        if not 1 <= self.A <= _lib.STOPSIGN_PER_MAX:
            raise ValueError('stop_signs: a junction holds 1 .. %d agents, the batch has A = %d' % (_lib.STOPSIGN_PER_MAX, self.A))
        if len({t is None for t in (stop, move, exit)}) > 1:
            raise ValueError('stop_signs: give stop, move and exit, or none of them')
        stop, move, exit = self._line_tables('stop_signs', (stop, move, exit), movement_lines)
        if conflict is None or lane is None:
            if conflict is not None or lane is not None:
                raise ValueError('stop_signs: give both conflict and lane, or neither')
            conflict, lane = movement_conflicts(self._route_list(), stop, exit, np.asarray(self.ip.circle_centers), float(self.ip.radius))
        conflict, lane = np.asarray(conflict), np.asarray(lane)
        n_moves = len(conflict)
        if (conflict.ndim != 1 or lane.shape != conflict.shape or not 1 <= n_moves <= _lib.SIGNAL_GROUPS_MAX or
                not np.issubdtype(conflict.dtype, np.integer) or not np.issubdtype(lane.dtype, np.integer)):
            raise ValueError('stop_signs: conflict and lane hold one integer word per movement, 1 .. %d movements' % _lib.SIGNAL_GROUPS_MAX)
        if signed is None:
            sign = np.ones(n_moves, np.int32)
        else:
            sign = np.asarray(signed)
            if sign.shape != (n_moves,):    # (arms, not one word per movement)
                if n_moves % 3:
                    raise ValueError('stop_signs: signed names arms, and %d movements are not three per arm' % n_moves)
                sign = sign_table(signed, n_moves // 3)
        if sign.shape != (n_moves,) or not np.issubdtype(sign.dtype, np.integer) or not np.isin(sign, (0, 1)).all():
            raise ValueError('stop_signs: signed is None, the arms that carry signs, or one 0 / 1 word per movement (%d)' % n_moves)
        gap = np.broadcast_to(np.asarray(gap, dtype=np.float64), (n_moves,)) if np.ndim(gap) == 0 else np.asarray(gap, dtype=np.float64)
        if gap.shape != (n_moves,) or not np.isfinite(gap).all() or (gap < 0).any():
            raise ValueError('stop_signs: gap is a finite, non-negative number of seconds, or one per movement (%d)' % n_moves)
        v_stop, v_floor, brake, patience = float(v_stop), float(v_floor), self._brake(brake), int(patience)
        if not (np.isfinite(v_stop) and v_stop > 0 and np.isfinite(v_floor) and v_floor > 0 and np.isfinite(brake) and brake > 0):
            raise ValueError('stop_signs: v_stop, v_floor and brake are finite and positive')
        zone = int(np.ceil(4.0 / self.dl)) if zone is None else int(zone)
        detect = max(int(stop.max()) if len(stop) else 1, zone) if detect is None else int(detect)
        if not 1 <= zone <= detect <= int(np.iinfo(np.int32).max) or not 0 <= patience <= int(np.iinfo(np.int32).max):
            raise ValueError('stop_signs: 1 <= zone <= detect path points and patience >= 0 steps, int32')
        if self._braking is not None and not zone * self.dl > self._braking.setback:
            raise ValueError('stop_signs: zone = %d points = %g m does not exceed the firm hold\'s setback of %g m: a car standing on its firm '
                             'stop point could never stamp its stop' % (zone, zone * self.dl, self._braking.setback))
        self._off('priority')       # (a junction is run by priority or by signs)
        c = self.ctx
        tabs = dict(path_stop=c.i32(stop), path_move=c.i32(move), path_exit=c.i32(exit), conflict=c.i32(conflict), lane=c.i32(lane),
                    sign=c.i32(sign), gap=torch.as_tensor(np.ascontiguousarray(gap), dtype=torch.float64, device=c.device))
        zeros = lambda n: torch.zeros(n, dtype=torch.int32, device=c.device)
        self.stopping, self.released, self.sign_clock, self.ran_sign = zeros(self.P), zeros(self.P), zeros(self.B), zeros(self.B)
        self.sign_occupied, self.n_waiting = zeros(self.B), zeros(self.B)
        self.stopped_at = torch.full((self.P,), -1, dtype=torch.int32, device=c.device)
        self.sign_blocker = torch.full((self.P,), -1, dtype=torch.int32, device=c.device)
        self.sign_lag = torch.full((self.P,), float('inf'), dtype=torch.float64, device=c.device)
        self._stopsign_tabs = tabs
        self._stopsign = _lib.StopSignC(tabs['path_stop'].data_ptr(), tabs['path_move'].data_ptr(), tabs['path_exit'].data_ptr(),
                                        tabs['conflict'].data_ptr(), tabs['lane'].data_ptr(), tabs['sign'].data_ptr(), tabs['gap'].data_ptr(),
                                        self.stopped_at.data_ptr(), self.released.data_ptr(), self.stopping.data_ptr(),
                                        self.sign_clock.data_ptr(), self.ran_sign.data_ptr(), self.sign_lag.data_ptr(),
                                        self.sign_blocker.data_ptr(), self.sign_occupied.data_ptr(), self.n_waiting.data_ptr(), v_stop, brake,
                                        v_floor, zone, detect, patience, self.A, self.B, n_moves, int(self.path.shape[0]), 0)
        c.set_stopsign(None)        # (a new table may sit where an old one sat: the context checks the next struct it is given afresh)
        self._desc = None
        c.synchronize()

    def no_signs(self):
        """switch the stop signs off and nothing else: the batch enqueues exactly the launches of one that never had them (the stage's
        words keep what they hold and are no longer written)"""
        self._off('stopsign')

    def share_plans(self, share=None):
        """SHARED PLANS (mpcx_closed_loop_run_intent).  Every agent is seen by the others through a prediction of its pool row: the controls
        it applied in the last step, held for pred_steps frames -- the reference's prediction of a scripted car.  A sharing agent is seen
        on the plan it solved one step ago instead (its braking in front of a cut path, a stop line or an advised speed is in there): one
        more launch between the prediction and the conflict search re-rolls that plan into the agent's own pool row.  share: None = every
        agent; else a bool or int array of P, nonzero = the agent shares (mixed fleets).  An agent whose last solve failed, that is retired
        or whose row is out of the scene is predicted as ever.  Allocates `shared_frames` (zero) and drops the cached descriptor;
        keep_plans_private() switches it off."""
        if callable(self.exchange) or self.exchange == 'rccl':
            raise MpcxError('share_plans: not with an agent-sharded exchange (the other ranks\' rows arrive without their plans)')
        if share is None:
            flags = np.ones(self.P, np.int32)
        else:
            flags = np.asarray(share)
            if flags.shape != (self.P,) or flags.dtype.kind not in 'biu':
                raise ValueError('share_plans: share must be a bool or int array of P = %d, got shape %s dtype %s' % (self.P, flags.shape, flags.dtype))
            flags = (flags != 0).astype(np.int32)
        dev = self.ctx.device
        self.share = torch.from_numpy(np.ascontiguousarray(flags)).to(dev)
        self.shared_frames = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self._intent = _lib.IntentC(self.share.data_ptr(), self.shared_frames.data_ptr(), self.P, 0)
        self._desc = None
        self.ctx.synchronize()

    def keep_plans_private(self):
        """switch the shared plans off and nothing else: the batch enqueues exactly the launches of one that never shared (`shared_frames`
        keeps what it holds and is no longer written)"""
        self._off('intent')

    def actuate(self, controllers, ctrl_of=None, stop=None, group=None, brake: Optional[float] = None):
        """VEHICLE-ACTUATED SIGNALS (mpcx_closed_loop_run_actuated).  Every instance is a junction (n_per = A) with a controller on the
        device: the launch that holds agents at their stop lines first reduces, over the junction's agents, which signal groups have a car
        within `detect` path points of its line, advances the junction's state machine and takes the lights from it.  A phase is held at
        least min_green steps, extended while its own groups are called, ended when they have not been for `gap` steps or at max_green --
        but only if another phase is called --, followed by `amber` steps of amber and `all_red` of red for all; phases nobody calls are
        skipped.  The hold at the line is signalise()'s, which this call replaces as the source of the lights (and the reverse).
        controllers: one dict or a sequence of dicts, dict(phases=[[groups], ...], min_green, max_green, gap, amber, all_red, detect), the
        three per-phase values a scalar or one value per phase, the same number of phases in all (two_phase_controller() builds one);
        ctrl_of: the controller of every instance (B,), default 0 -- a sweep of timings runs as one batch.  stop, group: the
        per-path-point tables (default: stop_lines() of the batch's routes).  brake: default abs(MAX_DECEL) of the batch's parameters.
        Allocates `held`, `junction_state`, `lights`, `calls` (zero) and the tables and drops the cached descriptor; unsignalise()
        switches it off."""
        if isinstance(controllers, dict):
            controllers = [controllers]
        controllers = list(controllers)
        if not controllers:
            raise ValueError('actuate: at least one controller')
        n_phases = len(controllers[0]['phases'])
        if not 1 <= n_phases <= _lib.ACTUATION_PHASES_MAX or any(len(ct['phases']) != n_phases for ct in controllers):
            raise ValueError('actuate: 1 .. %d phases, the same number in all controllers' % _lib.ACTUATION_PHASES_MAX)
        masks = np.zeros((len(controllers), n_phases), dtype=np.int64)
        times = np.zeros((len(controllers), n_phases, 3), dtype=np.int64)
        ctrl = np.zeros((len(controllers), 3), dtype=np.int64)
        for k, ct in enumerate(controllers):
            for p, groups in enumerate(ct['phases']):
                groups = [int(g) for g in groups]
                if not groups or any(not 0 <= g < _lib.SIGNAL_GROUPS_MAX for g in groups):
                    raise ValueError('actuate: controller %d phase %d: at least one signal group, each 0 .. %d' % (k, p, _lib.SIGNAL_GROUPS_MAX - 1))
                masks[k, p] = sum(1 << g for g in set(groups))
            for col, name in enumerate(('min_green', 'max_green', 'gap')):
                v = np.asarray(ct[name])
                if not np.issubdtype(v.dtype, np.integer) or v.shape not in ((), (n_phases,)):
                    raise ValueError('actuate: controller %d: %s is an integer or one integer per phase' % (k, name))
                times[k, :, col] = v
            ctrl[k] = [int(ct['amber']), int(ct['all_red']), int(ct['detect'])]
        stop, group = self._line_tables('actuate', (stop, group), stop_lines)
        # the signal groups: every group a phase or a path point names (a point with a group beyond the limit is a defective entry: free)
        n_groups = min(max(int(masks.max()).bit_length(), int(group.max()) + 1 if len(group) else 1), _lib.SIGNAL_GROUPS_MAX)
        ctrl_of, brake = self._per_instance('actuate', 'ctrl_of', ctrl_of), self._brake(brake)
        c = self.ctx
        tabs = dict(path_stop=c.i32(stop), path_group=c.i32(group), phase_groups=c.i32(masks), phase_time=c.i32(times), ctrl_time=c.i32(ctrl),
                    ctrl_of=c.i32(ctrl_of))
        self.held = torch.zeros(self.P, dtype=torch.int32, device=c.device)
        self.junction_state = torch.zeros((self.B, 4), dtype=torch.int32, device=c.device)
        self.lights = torch.zeros(self.B, dtype=torch.int32, device=c.device)
        self.calls = torch.zeros(self.B, dtype=torch.int32, device=c.device)
        self._planless_signals(tabs, brake, n_groups)
        self._actuation = _lib.ActuationC(tabs['phase_groups'].data_ptr(), tabs['phase_time'].data_ptr(), tabs['ctrl_time'].data_ptr(),
                                          tabs['ctrl_of'].data_ptr(), self.junction_state.data_ptr(), self.lights.data_ptr(),
                                          self.calls.data_ptr(), self.A, self.B, n_phases, len(controllers), 0)
        self._off('advice', 'reservation', 'priority', 'stopsign')  # (a junction is run by lights, by a manager, or by priority; there is no plan left to look ahead into; a controller replaces a junction manager)
        c.synchronize()

    def reserve(self, managers, manager_of=None, stop=None, group=None, exit=None, conflict=None, lane=None, brake: Optional[float] = None):
        """CROSSING RESERVATIONS (mpcx_closed_loop_run_reserved).  Every instance is a junction (n_per = A <= 64) with a manager on the
        device.  The movement of a car is the signal group of its stop line; a car within `detect` path points of its line requests the
        crossing, and the launch that holds agents at their stop lines grants the requests in the order of their first request (ties: the
        nearer car, then the lower agent index): a request is granted if its movement conflicts with no movement that holds the crossing --
        a car inside it or one that holds a grant -- and no car of its own approach lane has just been denied in front of it.  A denied
        request that has waited `patience` steps also blocks every later request that conflicts with it: patience 0 is strict first come,
        first served, patience None (unbounded) lets every compatible car pass a waiting one.  A grant is never revoked; a car gives the
        crossing back at its exit point.  The hold at the line is signalise()'s, which this call replaces as its source (and the reverse,
        as with actuate()); advice is dropped.
        managers: one dict(detect, patience) or a sequence of them; manager_of: the manager of every instance (B,), default 0 -- a sweep
        runs as one batch.  stop, group, exit: the per-path-point tables (default: movement_lines() of the batch's routes); conflict, lane:
        one bit mask per movement (default: movement_conflicts() of the batch's routes with the batch's disc model).  brake: unused by the
        rule (there is no amber), default abs(MAX_DECEL).
        Allocates `held`, `granted`, `queued`, `occupied`, `junction_clock` (zero), `since` (-1) and the tables and drops the cached
        descriptor; unsignalise() switches it off."""
        if isinstance(managers, dict):
            managers = [managers]
        managers = list(managers)
        if not managers:
            raise ValueError('reserve: at least one manager')
        if not 1 <= self.A <= _lib.RESERVE_PER_MAX:
            raise ValueError('reserve: a junction holds 1 .. %d agents, the batch has A = %d' % (_lib.RESERVE_PER_MAX, self.A))
        big = int(np.iinfo(np.int32).max)
        times = np.array([[int(m['detect']), big if m.get('patience') is None else int(m['patience'])] for m in managers], dtype=np.int64)
        if (times[:, 0] < 1).any() or (times[:, 1] < 0).any() or (times > big).any():
            raise ValueError('reserve: detect >= 1 path point, patience >= 0 steps or None, both int32')
        stop, group, exit = self._line_tables('reserve', (stop, group, exit), movement_lines)
        if conflict is None or lane is None:
            if conflict is not None or lane is not None:
                raise ValueError('reserve: give both conflict and lane, or neither')
            conflict, lane = movement_conflicts(self._route_list(), stop, exit, np.asarray(self.ip.circle_centers), float(self.ip.radius))
        conflict, lane = np.asarray(conflict), np.asarray(lane)
        n_groups = len(conflict)
        if conflict.ndim != 1 or lane.shape != conflict.shape or not 1 <= n_groups <= _lib.SIGNAL_GROUPS_MAX:
            raise ValueError('reserve: conflict and lane hold one word per movement, 1 .. %d movements' % _lib.SIGNAL_GROUPS_MAX)
        manager_of, brake = self._per_instance('reserve', 'manager_of', manager_of), self._brake(brake)
        c = self.ctx
        tabs = dict(path_stop=c.i32(stop), path_group=c.i32(group), path_exit=c.i32(exit), conflict=c.i32(conflict), lane=c.i32(lane),
                    mgr_time=c.i32(times), mgr_of=c.i32(manager_of))
        zeros = lambda n: torch.zeros(n, dtype=torch.int32, device=c.device)
        self.held, self.granted = zeros(self.P), zeros(self.P)
        self.since = torch.full((self.P,), -1, dtype=torch.int32, device=c.device)
        self.junction_clock, self.occupied, self.queued = zeros(self.B), zeros(self.B), zeros(self.B)
        self._planless_signals(tabs, brake, n_groups)
        self._reservation = _lib.ReservationC(tabs['path_exit'].data_ptr(), tabs['conflict'].data_ptr(), tabs['lane'].data_ptr(),
                                              tabs['mgr_time'].data_ptr(), tabs['mgr_of'].data_ptr(), self.granted.data_ptr(),
                                              self.since.data_ptr(), self.junction_clock.data_ptr(), self.occupied.data_ptr(),
                                              self.queued.data_ptr(), self.A, self.B, len(managers), 0)
        self._off('actuation', 'advice', 'keepclear', 'priority', 'stopsign')   # (a junction is run by lights, by a manager, or by priority; a junction manager replaces a controller or a plan; there is no plan to look ahead into; the manager itself keeps the crossing clear)
        c.synchronize()

    def unsignalise(self):
        """switch the signals off, fixed or actuated -- and the advice that draws on them -- and nothing else: the batch enqueues exactly the launches of one that never had them
        (`tick`, `held` and the junction words keep what they hold and are no longer read or written)"""
        self._off('signals')                # (advice looks ahead into the signals' plan)

    def stop_respawning(self):
        """switch respawn off and nothing else: the batch enqueues exactly the launches of one with admission alone.  Vehicles in flight
        finish (and stay departed), waiting ones still enter; `served` and the episode table keep what they hold.  Routing goes with it: a
        slot keeps the route its last reset gave it"""
        self._off('respawn')

    def served_count(self) -> int:
        """episodes finished so far, over all slots (one small reduction and one synchronisation)"""
        if self.served is None:
            raise MpcxError('served_count(): respawn_on_schedule() has not been called')
        return int(self.served.sum().item())

    def episodes(self) -> np.ndarray:
        """one row per finished episode, slot-major (EPISODE_DTYPE; synchronises): slot, generation, due, entered, arrived (step indices
        counted from respawn_on_schedule()), steps_driven (= arrived - entered + 1), delay = entered - due -- what the gate and the slot's
        previous vehicle held it back for --, and, with a run log attached (else False, +inf, -1, -1): contact, min_clearance as RunLog defines
        them for the episode, and row_begin, row_end: the episode's rows are RunLog.rows(slot)[row_begin:row_end]"""
        if self.served is None:
            raise MpcxError('episodes(): respawn_on_schedule() has not been called')
        self.ctx.synchronize()
        served, w, f = self.served.cpu().numpy(), self.ep_i32.cpu().numpy(), self.ep_f64.cpu().numpy()
        q, g = np.nonzero(np.arange(w.shape[1])[None, :] < served[:, None])
        out = np.zeros(len(q), EPISODE_DTYPE)
        rec = {n: w[q, g, k] for k, n in enumerate(_lib.EPISODE_I32)}
        out['slot'], out['generation'] = q, g
        for n in ('due', 'entered', 'arrived', 'steps_driven', 'row_end'):
            out[n] = rec[n]
        out['delay'] = rec['entered'] - rec['due']
        out['contact'] = rec['contact_step'] >= 0
        out['min_clearance'] = f[q, g, 0]
        out['row_begin'] = np.where(rec['row_end'] >= 0, rec['row_end'] - rec['steps_driven'], -1)
        return out

    def episode_routes(self) -> np.ndarray:
        """the route of every finished episode, aligned with the rows of episodes() (int32; synchronises): word 7 of the episode record,
        which a routed run writes (without routes it is 0 for every episode)"""
        if self.served is None:
            raise MpcxError('episode_routes(): respawn_on_schedule() has not been called')
        self.ctx.synchronize()
        served, w = self.served.cpu().numpy(), self.ep_i32.cpu().numpy()
        q, g = np.nonzero(np.arange(w.shape[1])[None, :] < served[:, None])
        return w[q, g, _lib.EPISODE_ROUTE_WORD].astype(np.int32)

    def movement_summary(self) -> np.ndarray:
        """the per-movement table of a routed run, reduced on the device (mpcx_episode_summary; one small launch, (B, R) records back instead
        of the P G records of the episode table; synchronises): a structured array (B, R) of MOVEMENT_DTYPE -- per instance and route, over
        the finished episodes on that route: count, contacts (episodes with a contact), delay_sum (sum of entered - due), steps_driven_sum,
        and min_clearance (the minimum over them; +inf if there are none or without a run log)"""
        if self.route_of is None:
            raise MpcxError('movement_summary(): respawn_on_schedule(route=...) has not been called')
        R = len(self._route_offs) - 1
        out_i, out_f = self.ctx.episode_summary(self.A, R, self.served, self.ep_i32, self.ep_f64)
        self.ctx.synchronize()
        out = np.zeros((self.B, R), MOVEMENT_DTYPE)
        wi = out_i.cpu().numpy()
        for k, n in enumerate(_lib.SUMMARY_I64):
            out[n] = wi[..., k]
        out['min_clearance'] = out_f.cpu().numpy()
        return out

    def waiting_count(self) -> int:
        """agents scheduled and not yet in (one small reduction and one synchronisation); 0 with admission off"""
        if self._admit is None:
            return 0
        return int((self.wait >= 0).sum().item())

    def entry_delay(self) -> np.ndarray:
        """(P,) steps between the step an agent was scheduled for and the step it entered in -- what the gate held it back for; 0 for
        agents present from the start, -1 for agents not yet in (synchronises)"""
        if self.entered_step is None:
            raise MpcxError('entry_delay(): enter_on_schedule() has not been called')
        self.ctx.synchronize()
        e = self.entered_step.cpu().numpy().astype(np.int64)
        return np.where(e >= 0, e - self.scheduled_step, -1)

    def active_count(self) -> int:
        """agents still driving (one small reduction and one synchronisation)"""
        if self._retire is None:
            return self.P
        return int((self.done == 0).sum().item())

    def run_until_done(self, max_steps: int, chunk: int = 16, graph: bool = False) -> int:
        """run(chunk) until every agent has arrived (active_count() == 0; with admission on: and nobody is waiting to enter,
        waiting_count() == 0) or max_steps have been taken; returns the steps taken.  The
        count is read back once per chunk, so a chunk may take up to chunk - 1 steps after the last arrival: each costs a near-empty
        launch sequence and changes nothing but the scripted cars."""
        if self._retire is None:
            raise MpcxError('run_until_done: retirement is off (retire_at_goal() first): nothing ever ends the run')
        if chunk < 1:
            raise ValueError('run_until_done: chunk must be >= 1')
        taken = 0
        while taken < max_steps and (self.active_count() > 0 or self.waiting_count() > 0):
            n = min(int(chunk), int(max_steps) - taken)
            self.run(n, graph)
            taken += n
        return taken

    def _descriptor(self) -> '_lib.ClosedLoopC':
        d = _lib.ClosedLoopC()
        d.P, d.exchange, d.dl = self.P, (_lib.SHARD_AGENTS if self.exchange == 'rccl' else 0), self.dl
        d.n_inst, d.agents_local = self.B, self.A
        d.obs_local = None if self.obs_local is None else self.obs_local.data_ptr()
        bufs = dict(state=self.state, applied=self.applied, obs6=self.obs6, path_xyyaw=self.path, path_cs=self.path_cs,
                    path_v=self.path_v, path_off=self.path_off, path_len=self.path_len, obs_off=self.obs_off,
                    obs_cnt=self.obs_cnt, obs_skip=self.obs_skip, traj_idx=self.traj_idx, target_ind=self.target_ind,
                    hit_idx=self.inter['hit_idx'], cut_len=self.inter['cut_len'], hit_xy=self.inter['hit_xy'],
                    xref=self.pre['xref'], xbar=self.pre['xbar'], reaches_end=self.pre['reaches_end'],
                    x_sol=self.sol['x'], u_sol=self.sol['u'], status=self.sol['status'], iters=self.sol['iters'],
                    kkt=self.sol['kkt'])
        for k, t in bufs.items():
            setattr(d, k, None if t is None else t.data_ptr())
        if self.traffic is not None and self.traffic.n_actors:
            d.n_actors, d.pool_rows = self.traffic.n_actors, int(self.obs6.shape[0])
            d.actors, d.actor_state, d.actor_row, d.ego_row = (t.data_ptr() for t in (self.actors, self.traffic_state, self.actor_row, self.ego_row))
            d.tape, d.tape_rows = (None, 0) if self.tape is None else (self.tape.data_ptr(), int(self.tape.shape[0]))
        return d

    def _claim_context(self):
        """the kernels size every access from the context's horizon: another MPC / batch on the same Context may have
        changed it since this batch was built"""
        if self.ctx.params != self.params:
            self.ctx.set_mpc_params(self.params)
        if getattr(self.ctx, 'lin_passes', 1) != self.lin_passes:
            self.ctx.set_linearisation_passes(self.lin_passes)
        self.ctx.set_instance_tuning(self.tuning)
        self.ctx.set_following(self._following)
        self.ctx.set_safety(self._safety)
        self.ctx.set_sight(self._sight)
        self.ctx.set_keepclear(self._keepclear)
        self.ctx.set_priority(self._priority)
        self.ctx.set_stopsign(self._stopsign)
        self.ctx.set_braking(self._braking)

    def run(self, n_steps: int, graph: bool = False):
        """n_steps of the closed loop with no host work in between (mpcx_closed_loop_run)."""
        if self._retire is not None and self.lin_passes > 1:
            raise MpcxError('retirement at the goal with lin_passes = %d: the later linearisation passes build their work queue without '
                            'the retired mask (MPCX_E_INVALID); keep_driving() or lin_passes = 1' % self.lin_passes)
        if self._intent is not None and (callable(self.exchange) or self.exchange == 'rccl'):
            raise MpcxError('shared plans with an agent-sharded exchange: the other ranks\' rows arrive without their plans; keep_plans_private()')
        if callable(self.exchange):          # rehearsal exchange (torch.distributed): the host moves the rows between stages
            if self._retire is not None:
                raise MpcxError('retirement at the goal%s with a callable exchange: it steps through step_staged(), whose per-stage entry '
                                'points have no retired mask; use exchange=\'rccl\' or keep_driving()' % (' (and admission)' if self._admit is not None else ''))
            for _ in range(n_steps):
                self.step_staged()
            return
        if (self._precedence is not None and self._precedence.mode == _lib.PRECEDENCE_ENTRY and
                self.steps_done + int(n_steps) > _lib.PRECEDENCE_MAX_STEP):
            raise MpcxError('give_way(order=\'entry\'): step %d is beyond the last step whose entry-order word fits int32 (%d)'
                            % (self.steps_done + int(n_steps), _lib.PRECEDENCE_MAX_STEP))
        if self._desc is None:
            self._desc = self._descriptor()
        self._claim_context()
        self.ctx.closed_loop_run(self.ip, self._desc, n_steps, graph, **self._stage_structs())
        self.steps_done += n_steps

    def step(self):
        self.run(1)

    def check(self):
        """Raise where the reference raises: Exception('something wrong') of calc_nearest_index_in_direction
        (trajectories.py:120; hit_idx -3 / target_ind -1) and the capacity limits of the interaction kernel (hit_idx -2:
        more than MPCX_MAX_REMAINING path points ahead, MPCX_EGO_FRAMES_MAX resampled poses or MPCX_MAX_OBS obstacles)
        -- in all of which the kernel leaves the agent's path uncut.  One small reduction + sync; call it every N steps."""
        bad = torch.stack([(self.inter['hit_idx'] == -2).sum(), (self.inter['hit_idx'] == -3).sum(), (self.target_ind < 0).sum()]).cpu().numpy()
        if bad.any():
            raise MpcxError('closed loop: %d agents beyond the interaction kernel\'s capacity (hit_idx -2), %d + %d nearest-index failures '
                            '("something wrong", trajectories.py:120) in the conflict search / reference window' % tuple(int(b) for b in bad))

    def step_staged(self):
        """the same step through the per-stage entry points (one host call per stage)"""
        if self._retire is not None:
            raise MpcxError('step_staged() with retirement at the goal%s: the per-stage entry points have no retired mask; run() or keep_driving()'
                            % (' and admission' if self._admit is not None else ''))
        if self._intent is not None and self.obs_local is not None:
            raise MpcxError('step_staged() with shared plans in the agent-sharded layout: the other ranks\' rows arrive without their plans')
        c = self.ctx
        self._claim_context()
        # what MovingObstacle*.get() would return for every agent: (x, y, v, yaw, a, steer)
        rows = self.obs6 if self.obs_local is None else self.obs_local
        if self.traffic is not None and self.traffic.n_actors:
            if self.obs_local is not None:
                raise MpcxError('scripted traffic is not supported in the agent-sharded layout')
            # agents into their pool rows, then the scripted cars: get() into theirs and step() (mpc_intersection.py:118-122, 155-156)
            self.obs6[self.ego_row64] = torch.cat([self.state, self.applied[:, 1:2], self.applied[:, 0:1]], dim=1)
            c.traffic_step(self.actors, self.traffic_state, self.actor_row, self.obs6, tape=self.tape)
        else:
            rows[:, 0:2] = self.state[:, 0:2]
            rows[:, 2] = self.state[:, 2]
            rows[:, 3] = self.state[:, 3]
            rows[:, 4] = self.applied[:, 1]
            rows[:, 5] = self.applied[:, 0]
        if self.obs_local is not None:       # agent-sharded: every rank assembles the whole pool
            loc = self.obs_local.view(self.B, self.A, 6)
            if callable(self.exchange):
                self.obs6.copy_(self.exchange(loc).reshape(-1, 6))
            else:
                c.allgather_states(_lib.SHARD_AGENTS, loc, self.obs6)
        speed = self.stop_mode == 'speed'
        c.interaction(self.ip, self.state, self.path, self.path_cs, self.path_off, self.path_len,
                      self.prev_len if speed else self.inter['cut_len'], self.obs6, self.obs_off, self.obs_cnt, self.obs_skip,
                      self.traj_idx, out=self.inter, intent=self._intent, u_sol=self.sol['u'], status=self.sol['status'])
        if self._safety is not None:        # the safety stage: directly behind the conflict search, on the prediction it read, as in the loop
            c.safety_step(self.ip, self.state, self.path_off, self.traj_idx, self.obs6, self.obs_off, self.obs_cnt, self.obs_skip, self._safety)
        if self._reservation is not None:   # the reservation stage, in the place of the signal stage
            c.reserve_step(self.dl, self.state, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._signals, self._reservation)
        elif self._actuation is not None:   # the actuated signal stage, in the place of the signal stage
            c.actuated_step(self.dl, self.state, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._signals, self._actuation)
        elif self._signals is not None:     # the signal stage: between the conflict search and the window stage, as in the loop
            c.signal_step(self.dl, self.state, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._signals)
        if self._keepclear is not None:     # the keep-clear stage: behind the signal / actuated stage, on the held it left, as in the loop
            c.keepclear_step(self.dl, self.state, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._signals, self._keepclear)
        if self._priority is not None:      # the priority stage: in the hold's place, as in the loop
            c.priority_step(self.dl, self.state, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._priority)
        if self._stopsign is not None:      # the stop-sign stage: in the priority stage's place, as in the loop
            c.stopsign_step(self.dl, self.state, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._stopsign)
        if self._following is not None:     # the following stage: behind the signal stage, in front of the window stage, as in the loop
            c.follow_step(self.dl, _lib.STOP_SPEED if speed else _lib.STOP_CUT, self.state, self.path, self.path_off, self.path_len, self.traj_idx,
                          self.inter['cut_len'], self.obs6, self.obs_off, self.obs_cnt, self._following, obs_skip=self.obs_skip)
        firm = self._braking is not None
        if firm:        # the firm hold's mark: behind the last hold and the following stage, in front of the window stage, as in the loop
            if self.lin_passes != 1:
                raise MpcxError('braking: not supported with more than one linearisation pass (%d)' % self.lin_passes)
            stop, held, boxed, yielding = self._line_words()
            if stop is None:
                raise MpcxError('braking: the run has no source of stop lines (signals, actuation, a reservation, the priority road or stop signs)')
            c.brake_mark_step(self.dl, _lib.STOP_SPEED if speed else _lib.STOP_CUT, self.path_off, self.path_len, self.traj_idx, self.target_ind,
                              self._win_len, stop, self._braking, held=held, boxed=boxed, yielding=yielding)
        # the previous solution (zeros where the last solve failed or on the first step) is the warm start
        for it in range(self.lin_passes):       # lib/mpc.py:226-237: from the second pass on the previous pass's speeds space the window
            if speed:       # the whole path + the stop index (mpcx_mpc_prepare_batch_stop).  len_seen is a side effect the NEXT step
                            # relies on: the window kernel leaves the path length in prev_len, which the next interaction() reads
                c.prepare(self.state, self.sol['u'], self.path, self.path_off, self._win_len if firm else self.path_len, self.dl, self.target_ind,
                          out=self.pre, path_v=self.path_v, x_prev=self.sol['x'] if it else None, stop_idx=self.inter['cut_len'], v_ref=self.v_ref,
                          len_seen=self.prev_len)
                if self._advice is not None:    # the advice stage: between the window stage and the QP, as in the loop
                    c.advise_step(self.dl, self.path_off, self.path_len, self.traj_idx, self.inter['cut_len'], self._signals, self._advice,
                                  self.pre['xref'])
                if self._following is not None:     # the following clamp: behind the window stage (and the advice), as in the loop
                    c.follow_cap_step(self._following, self.pre['xref'])
                if firm:        # the firm hold's clamp: behind the window stage, beside the other clamps, as in the loop
                    c.brake_clamp_step(self.dl, self.state, self.path, self.path_off, self.path_len, self.traj_idx, stop, self._braking,
                                       self.pre['xref'], prev_len=self.prev_len)
            else:
                c.prepare(self.state, self.sol['u'], self.path, self.path_off, self.inter['cut_len'], self.dl, self.target_ind, out=self.pre,
                          path_v=self.path_v, x_prev=self.sol['x'] if it else None)
            c.qp_solve(self.state, self.pre['xref'], self.pre['xbar'], self.pre['reaches_end'], self.sol['u'], out=self.sol)
        c.plant_step(self.state, self.sol['u'], self.sol['status'], self.applied)
        if self.log is not None:
            c.record_step(self.ip, self.state, self.applied, self.sol['x'], self.path, self.path_off, self.path_len, self.target_ind,
                          self.inter['cut_len'], self.traj_idx, self.inter['hit_idx'], self.sol['status'], self.sol['iters'], self.obs6,
                          self.obs_off, self.obs_cnt, self.obs_skip, self.log.c, goal_len=self.path_len if speed else None)
        self.steps_done += 1

    def snapshot(self):
        """host copies of the per-agent state (synchronises)"""
        self.ctx.synchronize()
        keys = ('state', 'applied', 'traj_idx', 'target_ind')
        out = {k: getattr(self, k).cpu().numpy().copy() for k in keys}
        out['prev_cut'] = (self.prev_len if self.stop_mode == 'speed' else self.inter['cut_len']).cpu().numpy().copy()
        out.update({k: v.cpu().numpy().copy() for k, v in self.sol.items()})
        out.update({k: v.cpu().numpy().copy() for k, v in self.inter.items()})
        out.update({k: v.cpu().numpy().copy() for k, v in self.pre.items()})
        if self.traffic is not None:         # the actors' states (x, y, theta, counter / cursor) and the pool as the last step saw it
            out['traffic_state'] = self.traffic_state.cpu().numpy().copy()
            out['obs6'] = self.obs6.cpu().numpy().copy()
        for st, words in _SNAPSHOT_WORDS.items():
            if getattr(self, '_' + st) is not None:
                out.update({key: getattr(self, attr).cpu().numpy().copy() for key, attr in words})
        if self._following is not None:      # the leader's pool row (-1 = none), the distance to it and the safe speed behind it, last step's
            out.update(leader=self.leader.cpu().numpy().copy(), gap=self.gap.cpu().numpy().copy(), follow_cap=self.follow_cap.cpu().numpy().copy())
        if self._braking is not None:        # the stop index of an agent held firmly at its line, its overruns so far, the profile at the window's head
            out.update(firm=self.firm.cpu().numpy().copy(), overran=self.overran.cpu().numpy().copy(), brake_cap=self.brake_cap.cpu().numpy().copy())
        if self._safety is not None:         # the nearest vehicle and the first predicted contact of the last step, the encounters so far
            out.update(partner=self.partner.cpu().numpy().copy(), near_clearance=self.near_clearance.cpu().numpy().copy(),
                       ttc_row=self.ttc_row.cpu().numpy().copy(), ttc_frame=self.ttc_frame.cpu().numpy().copy(),
                       n_events=self.n_events.cpu().numpy().copy())
        if self._sight is not None:          # who saw whom in the last step: the uint64 word per agent and its two counts
            out.update(sight=self.sight.cpu().numpy().view(np.uint64).copy(), n_seen=self.n_seen.cpu().numpy().copy(),
                       n_hidden=self.n_hidden.cpu().numpy().copy())
        if self._keepclear is not None:      # who was kept at its line in the last step, who stood there, and the movements inside per junction
            out.update(boxed=self.boxed.cpu().numpy().copy(), box_waited=self.box_waited.cpu().numpy().copy(),
                       box_occupied=self.box_occupied.cpu().numpy().copy(), n_boxed=self.n_boxed.cpu().numpy().copy())
        if self._priority is not None:       # who was kept at its line in the last step, for whom and by what lag, and the movements inside per junction
            out.update(yielding=self.yielding.cpu().numpy().copy(), yield_waited=self.yield_waited.cpu().numpy().copy(),
                       blocker=self.blocker.cpu().numpy().copy(), lag=self.lag.cpu().numpy().copy(),
                       crossing=self.crossing.cpu().numpy().copy(), n_yielding=self.n_yielding.cpu().numpy().copy())
        if self._stopsign is not None:       # who was held at its line in the last step, who has stopped and when, who has been released, the cars that ran a sign
            out.update(stopping=self.stopping.cpu().numpy().copy(), stopped_at=self.stopped_at.cpu().numpy().copy(),
                       released=self.released.cpu().numpy().copy(), ran_sign=self.ran_sign.cpu().numpy().copy())
        if self._routes is not None:        # the route every slot is on now: the run of the path tables its path_off names
            out['route'] = (np.searchsorted(self._route_offs, self.path_off.cpu().numpy().astype(np.int64), side='right') - 1).astype(np.int32)
        if self._actuation is not None:      # per junction: the state the NEXT step starts from, and the lights the last step showed
            js = self.junction_state.cpu().numpy()
            out['phase'], out['stage'], out['lights'] = js[:, 0].copy(), js[:, 1].copy(), self.lights.cpu().numpy().copy()
        return out

    def stop_index(self) -> np.ndarray:
        """speed mode: the agents' stop indices of the last step in the reference's own terms (the `cutoff_idx` of
        mpc_intersection_new_ref.py:122-139): the conflict search's cut index where it found a conflict, _lib.NO_STOP (999) where it
        did not (synchronises).  The device keeps the path length for "no conflict" -- a stop index nothing reaches.  With signals on, an
        agent held at its stop line (held != 0) reports its stop index too: the line, or a conflict in front of it."""
        if self.stop_mode != 'speed':
            raise MpcxError('stop_index(): the batch runs with stop_mode=%r' % self.stop_mode)
        self.ctx.synchronize()
        stops = self.inter['hit_idx'].cpu().numpy() >= 0
        if self._signals is not None:
            stops = stops | (self.held.cpu().numpy() != 0)
        if self._following is not None:     # (the stop point behind a leader lies on the path whenever there is a leader)
            stops = stops | (self.leader.cpu().numpy() >= 0)
        return np.where(stops, self.inter['cut_len'].cpu().numpy(), _lib.NO_STOP).astype(np.int32)


def corner_blocks(setback: float = 5.0, extent: float = 42.0):
    """the four corner buildings of the stock four-way world as BoxObstacles: squares of side `extent` whose inner corners stand at
    (+-setback, +-setback) -- the occluders of IntersectionBatch.occlude() for a blind junction.  The world's own obstacle list is not a good
    occluder set as it stands: it also holds the medians and the hidden=True wrong-way lanes."""
    from .lib.obstacles import BoxObstacle
    c = float(setback) + float(extent) / 2.0
    return [BoxObstacle(xy_width=(float(extent), float(extent)), height=0.5, xy_center=(sx * c, sy * c)) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def _convex_box(rows: np.ndarray):
    """the bounding box (x0, y0, x1, y1) of the convex polygon {a x + b y + c <= 0 for all rows}: over the pairwise intersections of its
    lines that satisfy every row (to 1e-9 of the rows' scale); None for an empty or unbounded one"""
    pts = []
    n = len(rows)
    for i in range(n):
        for j in range(i + 1, n):
            m = np.array([rows[i, :2], rows[j, :2]])
            det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
            if det == 0.0:
                continue
            p = np.array([(-rows[i, 2] * m[1, 1] + rows[j, 2] * m[0, 1]) / det, (-rows[j, 2] * m[0, 0] + rows[i, 2] * m[1, 0]) / det])
            if (rows[:, :2] @ p + rows[:, 2] <= 1e-9 * (1.0 + np.abs(rows).max())).all():
                pts.append(p)
    if len(pts) < 2:
        return None
    pts = np.array(pts)
    return np.array([pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()])


def occluder_table(obstacle_lists, shrink: float = 0.0):
    """the occluder tables of mpcx_sight for a list of obstacle lists (one list = one set): (hp, hp_off, box, set_off) -- hp (rows, 3)
    float64, the half-plane rows to_convex(-shrink) of every occluder, inside <=> a x + b y + c <= 0; hp_off (n_occ + 1,) int32; box
    (n_occ, 4) float64, (x0, y0, x1, y1) of every occluder; set_off (n_sets + 1,) int32.  An occluder that the shrink leaves empty is
    dropped."""
    hp, hp_off, box, set_off = [], [0], [], [0]
    for obstacles in obstacle_lists:
        for o in obstacles:
            rows = np.asarray(o.to_convex(-float(shrink)), dtype=np.float64).reshape(-1, 3)
            bb = _convex_box(rows)
            if bb is None:
                continue
            hp.append(rows); box.append(bb); hp_off.append(hp_off[-1] + len(rows))
        set_off.append(len(box))
    return (np.concatenate(hp) if hp else np.zeros((0, 3)), np.asarray(hp_off, np.int32), np.array(box, dtype=np.float64).reshape(-1, 4),
            np.asarray(set_off, np.int32))


def stop_lines(routes, half_width: float = 12.0, setback: float = 6.0):
    """The two per-path-point tables of IntersectionBatch.signalise for `routes` (a list of (n, 3) paths, concatenated in order as the batch
    concatenates them): (path_stop, path_group), int32, one word per path point.  The crossing is the square max(|x|, |y|) <= half_width
    about the origin (the stock crossing: distance_center 12).  The stop line of a route is the last point that lies at least `setback`
    metres of arc before the route's first point inside the square; path_stop of every point up to and including the line is the line's
    route-local index, -1 behind it (and everywhere on a route that starts inside the square, never enters it or has no such point).  The
    signal group is the approach arm minus one, taken from the route's first point: 0 = from the south (y most negative; arm 1 of the stock
    scenario), 1 = from the west (arm 2), 2 = from the north (arm 3), 3 = from the east (arm 4).  path_group is the group on every point
    that has a line ahead, 0 elsewhere.  Pure numpy: no GPU, no state."""
    stop, group = [], []
    for r in routes:
        r = np.asarray(r, dtype=np.float64)
        n = len(r)
        st, gr = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
        inside = np.flatnonzero(np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) <= half_width)
        if n and len(inside) and inside[0] > 0:
            arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(r[:, 0]), np.diff(r[:, 1])))])
            ok = np.flatnonzero(arc[:inside[0]] <= arc[inside[0]] - setback)
            if len(ok):
                x0, y0 = r[0, 0], r[0, 1]
                arm = (0 if y0 < 0 else 2) if abs(y0) >= abs(x0) else (1 if x0 < 0 else 3)
                st[:ok[-1] + 1] = ok[-1]
                gr[:ok[-1] + 1] = arm
        stop.append(st); group.append(gr)
    if not stop:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    return np.concatenate(stop), np.concatenate(group)


def _arm_of(x: float, y: float) -> int:
    """the arm a point outside the crossing lies on: 0 south, 1 west, 2 north, 3 east (stop_lines()' signal groups)"""
    return (0 if y < 0 else 2) if abs(y) >= abs(x) else (1 if x < 0 else 3)


def _movement_of(r) -> int:
    """the movement index 3 (arm - 1) + (turn - 1) of a route, -1 for a route that leaves on the arm it came from: the approach arm from its
    first point, as in stop_lines(), the exit arm from its last; turn 1 / 2 / 3 = the exit arm is the next clockwise / the opposite one /
    the next anticlockwise as seen from above (south -> west -> north -> east is clockwise)"""
    arm, out = _arm_of(r[0, 0], r[0, 1]), _arm_of(r[-1, 0], r[-1, 1])
    turn = (out - arm) % 4
    return 3 * arm + turn - 1 if turn else -1


def movement_lines(routes, half_width: float = 12.0, setback: float = 6.0, clear: float = 4.0):
    """The three per-path-point tables of IntersectionBatch.reserve for `routes` (a list of (n, 3) paths, concatenated in order):
    (path_stop, path_group, path_exit), int32, one word per path point.  path_stop is that of stop_lines().  The exit point of a route is
    the first point at least `clear` metres of arc behind its last point inside the crossing square (the route's length if it ends before
    that); path_exit of every point before it is its route-local index, -1 from it on (and everywhere on a route that never enters the
    square or leaves on the arm it came from).  path_group of every point before the exit is the route's MOVEMENT, 3 (arm - 1) + (turn - 1)
    with the approach arm as in stop_lines() and turn 1 / 2 / 3 = the exit arm, taken from the route's last point, is the next clockwise /
    the opposite / the next anticlockwise one as seen from above -- the stock scenario's (start position, turn indicator) --, 0 elsewhere.
    Pure numpy: no GPU, no state."""
    stop, _ = stop_lines(routes, half_width, setback)
    group, exits = [], []
    for r in routes:
        r = np.asarray(r, dtype=np.float64)
        n = len(r)
        gr, ex = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
        inside = np.flatnonzero(np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) <= half_width) if n else np.zeros(0, dtype=np.int64)
        mv = _movement_of(r) if n else -1
        if len(inside) and mv >= 0:
            arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(r[:, 0]), np.diff(r[:, 1])))])
            ok = np.flatnonzero(arc >= arc[inside[-1]] + clear)
            e = int(ok[0]) if len(ok) else n
            ex[:e] = e
            gr[:e] = mv
        group.append(gr); exits.append(ex)
    if not group:
        return stop, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    return stop, np.concatenate(group), np.concatenate(exits)


def movement_conflicts(routes, stop, exit, circle_centers, radius: float, margin: float = 1.0):
    """The two movement tables of IntersectionBatch.reserve for `routes` with the tables of movement_lines(): (conflict, lane), int32, one
    word per movement of a four-arm crossing (12).  Two movements of different arms conflict (bit h of conflict[g] and bit g of conflict[h])
    if some disc centre of a route of the one, over its points [stop, exit) -- from its line, or its first point if it has none, to its
    exit --, comes within 2 radius + margin of some disc centre of a route of the other.  Movements of the same arm share a lane (lane[g] =
    the three movements of g's arm) and never conflict.  circle_centers: the discs' offsets along the vehicle's axis (2,), or (x, y)
    offsets in the vehicle's frame (2, 2) as the interaction parameters hold them.  Pure numpy: no GPU, no state."""
    cc = np.asarray(circle_centers, dtype=np.float64).reshape(-1)
    cc = np.column_stack([cc, np.zeros_like(cc)]) if cc.size == 2 else cc.reshape(-1, 2)
    stop, exit = np.asarray(stop), np.asarray(exit)
    swept = {}
    off = 0
    for r in routes:
        r = np.asarray(r, dtype=np.float64)
        n = len(r)
        mv = _movement_of(r) if n else -1
        if n and mv >= 0 and exit[off] >= 0:
            pts = r[max(int(stop[off]), 0):int(exit[off])]
            cs, sn = np.cos(pts[:, 2]), np.sin(pts[:, 2])
            discs = np.concatenate([np.column_stack([pts[:, 0] + ox * cs - oy * sn, pts[:, 1] + ox * sn + oy * cs]) for ox, oy in cc])
            swept.setdefault(mv, []).append(discs)
        off += n
    conflict = np.zeros(12, dtype=np.int64)
    lane = np.array([7 << 3 * (g // 3) for g in range(12)], dtype=np.int64)
    reach = 2.0 * float(radius) + float(margin)
    for g in swept:
        for h in swept:
            if g // 3 == h // 3 or h < g:
                continue
            a, b = np.concatenate(swept[g]), np.concatenate(swept[h])
            d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
            if len(a) and len(b) and d2.min() <= reach * reach:
                conflict[g] |= 1 << h
                conflict[h] |= 1 << g
    return conflict.astype(np.int32), lane.astype(np.int32)


def cross_phase_conflicts(conflict, phases=((0, 2), (1, 3))):
    """The conflict table of IntersectionBatch.keep_clear from movement_conflicts()' (one word per movement 3 (arm - 1) + (turn - 1)): bit h
    of word g is kept only if the arms g // 3 and h // 3 share no phase of `phases` (a sequence of sequences of arms = signal groups; the
    default is two_phase_plan()'s and two_phase_controller()'s).  Movements that are green together sort themselves out as ever -- a
    permissive turn against the opposed arm must not be blocked by it --; the contacts a two-phase plan leaves are between arms of
    different phases.  Symmetric if `conflict` is.  Pure numpy: no GPU, no state."""
    conflict = np.asarray(conflict, dtype=np.int64)
    together = {(a, b) for ph in phases for a in ph for b in ph}
    out = np.zeros_like(conflict)
    for g in range(len(conflict)):
        for h in range(len(conflict)):
            if (int(conflict[g]) >> h) & 1 and (g // 3, h // 3) not in together:
                out[g] |= 1 << h
    return out.astype(np.int32)


def priority_ranks(major=(0, 2), left_turn: int = 1):
    """The rank table of IntersectionBatch.priority_road for the twelve movements 3 arm + (turn - 1) of a four-arm crossing, int32 (12,): on
    an arm of `major` (arms 0 .. 3 = stop_lines()' signal groups) 1 for the turn `left_turn` and 0 otherwise, on the other arms 3 for that
    turn and 2 otherwise.  A smaller rank goes first: the major road's through and near-side traffic, its turn across the opposed stream, the
    minor road, the minor road's turn across.  With the stock routes turn 1 is the turn that crosses the opposed straight
    (movement_conflicts() has movement (arm 3, turn 1) against (arm 1, turn 2)).  Pure numpy: no GPU, no state."""
    major = {int(a) for a in major}
    if not major <= {0, 1, 2, 3} or left_turn not in (1, 2, 3):
        raise ValueError('priority_ranks: major holds arms 0 .. 3, left_turn is 1, 2 or 3')
    return np.array([(0 if g // 3 in major else 2) + (1 if g % 3 == left_turn - 1 else 0) for g in range(12)], dtype=np.int32)


def sign_table(signed=None, n_arms: int = 4):
    """The sign table of IntersectionBatch.stop_signs for the 3 n_arms movements 3 arm + (turn - 1) of a crossing, int32: 1 for every
    movement of an arm in `signed` (arms 0 .. n_arms - 1 = stop_lines()' signal groups), 0 for the others -- the through road.  signed =
    None: all-way, every movement carries a sign.  Pure numpy: no GPU, no state."""
    n_arms = int(n_arms)
    if not 1 <= n_arms or 3 * n_arms > _lib.SIGNAL_GROUPS_MAX:
        raise ValueError('sign_table: 1 .. %d arms of three movements each' % (_lib.SIGNAL_GROUPS_MAX // 3))
    arms = set(range(n_arms)) if signed is None else {int(a) for a in signed}
    if not arms <= set(range(n_arms)):
        raise ValueError('sign_table: signed holds arms 0 .. %d' % (n_arms - 1))
    return np.array([1 if g // 3 in arms else 0 for g in range(3 * n_arms)], dtype=np.int32)


def two_phase_plan(cycle: int, green: int, amber: int) -> dict:
    """A two-phase plan for the four signal groups of stop_lines(): dict(cycle, amber, green (4, 2)).  Groups 0 and 2 (arms 1 and 3, the
    south-north road) share the first phase, green from step 0; groups 1 and 3 (arms 2 and 4) share the second, green from step cycle // 2;
    each green lasts `green` steps and is followed by `amber` steps of amber.  What is left of a half cycle is the all-red gap that clears
    the crossing: cycle // 2 - green - amber >= 0 steps."""
    cycle, green, amber = int(cycle), int(green), int(amber)
    half = cycle // 2
    if cycle < 2 or green < 0 or amber < 0 or green + amber > half:
        raise ValueError('two_phase_plan: green + amber = %d + %d must fit half a cycle of %d steps' % (green, amber, cycle))
    return dict(cycle=cycle, amber=amber, green=np.array([[0, green], [half, green], [0, green], [half, green]], dtype=np.int32))


def two_phase_controller(min_green: int, max_green: int, gap: int, amber: int, all_red: int, detect: int) -> dict:
    """An actuated two-phase controller for the four signal groups of stop_lines(), for IntersectionBatch.actuate: phases [[0, 2], [1, 3]]
    -- the phases of two_phase_plan() --, every phase with the same (min_green, max_green, gap) in steps; `amber` steps of amber and
    `all_red` steps of red for all between phases; a car calls its group from `detect` path points before its line on."""
    v = dict(min_green=int(min_green), max_green=int(max_green), gap=int(gap), amber=int(amber), all_red=int(all_red), detect=int(detect))
    if v['min_green'] < 0 or v['max_green'] < 1 or v['min_green'] > v['max_green'] or v['gap'] < 1 or v['amber'] < 0 or v['all_red'] < 0 or v['detect'] < 1:
        raise ValueError('two_phase_controller: 0 <= min_green <= max_green, max_green >= 1, gap >= 1, amber >= 0, all_red >= 0, detect >= 1')
    return dict(phases=[[0, 2], [1, 3]], **v)


def entry_schedule(route_of_agent, routes, start_index, mean_headway_steps: float, seed: int) -> np.ndarray:
    """Seeded arrival times for IntersectionBatch.enter_on_schedule: a (B, A) integer `wait` array.  Per instance, the agents whose start
    poses coincide (the same route point x, y: e.g. the two stock routes of one approach arm, both from index 0) form one approach QUEUE, in
    agent order.  The k-th car of a queue is due at the cumulative sum of k + 1 draws of rng.geometric(1 / mean_headway_steps) - 1 -- memoryless
    headways with that mean (>= 1; 1 = everybody at once, all zeros) --, rng = numpy.random.default_rng(seed); draws are taken instance-major,
    queue by queue in the order of the queues' first agents.  Pure numpy and deterministic: no GPU, no state."""
    route_of_agent, start_index = np.asarray(route_of_agent, dtype=np.int64), np.asarray(start_index, dtype=np.int64)
    if route_of_agent.ndim != 2 or route_of_agent.shape != start_index.shape:
        raise ValueError('entry_schedule: route_of_agent and start_index must both have shape (B, A)')
    if not mean_headway_steps >= 1:
        raise ValueError('entry_schedule: mean_headway_steps must be >= 1')
    rng = np.random.default_rng(seed)
    B, A = route_of_agent.shape
    wait = np.zeros((B, A), dtype=np.int64)
    for b in range(B):
        pose = [tuple(float(v) for v in np.asarray(routes[route_of_agent[b, a]])[start_index[b, a], :2]) for a in range(A)]
        seen = []
        for a in range(A):
            if pose[a] in seen:
                continue
            seen.append(pose[a])
            queue = [k for k in range(A) if pose[k] == pose[a]]
            wait[b, queue] = np.cumsum(rng.geometric(1.0 / mean_headway_steps, size=len(queue)) - 1)
    return wait


def demand_schedule(route_of_agent, routes, start_index, mean_headway_steps: float, generations: int, seed: int) -> np.ndarray:
    """Seeded demand for IntersectionBatch.respawn_on_schedule: a (B, A, G) integer `due` array.  Per instance, the slots whose start poses
    coincide form one approach QUEUE, in agent order (as in entry_schedule).  A queue of n slots draws ONE memoryless arrival stream of n G
    vehicles -- the k-th is due at the cumulative sum of k + 1 draws of rng.geometric(1 / mean_headway_steps) - 1 -- and deals it to its slots
    in turn: vehicle k goes to slot k mod n as that slot's generation k div n, so every slot's due steps are non-decreasing.  rng =
    numpy.random.default_rng(seed); draws are taken instance-major, queue by queue in the order of the queues' first agents.  Pure numpy and
    deterministic: no GPU, no state."""
    route_of_agent, start_index = np.asarray(route_of_agent, dtype=np.int64), np.asarray(start_index, dtype=np.int64)
    if route_of_agent.ndim != 2 or route_of_agent.shape != start_index.shape:
        raise ValueError('demand_schedule: route_of_agent and start_index must both have shape (B, A)')
    if not mean_headway_steps >= 1:
        raise ValueError('demand_schedule: mean_headway_steps must be >= 1')
    G = int(generations)
    if G < 1:
        raise ValueError('demand_schedule: generations must be >= 1')
    rng = np.random.default_rng(seed)
    B, A = route_of_agent.shape
    due = np.zeros((B, A, G), dtype=np.int64)
    for b in range(B):
        pose = [tuple(float(v) for v in np.asarray(routes[route_of_agent[b, a]])[start_index[b, a], :2]) for a in range(A)]
        seen = []
        for a in range(A):
            if pose[a] in seen:
                continue
            seen.append(pose[a])
            queue = [k for k in range(A) if pose[k] == pose[a]]
            stream = np.cumsum(rng.geometric(1.0 / mean_headway_steps, size=len(queue) * G) - 1)
            due[b, queue, :] = stream.reshape(G, len(queue)).T
    return due


def turning_demand(route_of_agent, routes, start_index, share, generations: int, seed: int) -> np.ndarray:
    """Seeded turning movements for IntersectionBatch.respawn_on_schedule(route=...): a (B, A, G) integer `route` array.  The CANDIDATE routes
    of slot (b, a) are those whose point at the slot's start index equals the slot's start pose -- the point of its own route
    route_of_agent[b, a] at start_index[b, a] -- bit for bit in x, y and yaw: the routes of its approach arm, in route order.  Every vehicle
    of the slot draws one of them with probability share[r] / (sum of share over the candidates).  A slot with a single candidate makes no
    draw; the others draw their G vehicles at once, rng.choice(n candidates, size=G, p=...), rng = numpy.random.default_rng(seed), instance-
    major then slot-major.  share: one weight >= 0 per route; the candidates of a drawing slot must not all have weight 0.  Pure numpy and
    deterministic: no GPU, no state."""
    route_of_agent, start_index = np.asarray(route_of_agent, dtype=np.int64), np.asarray(start_index, dtype=np.int64)
    if route_of_agent.ndim != 2 or route_of_agent.shape != start_index.shape:
        raise ValueError('turning_demand: route_of_agent and start_index must both have shape (B, A)')
    R = len(routes)
    share = np.asarray(share, dtype=np.float64)
    if share.shape != (R,) or not np.isfinite(share).all() or (share < 0).any():
        raise ValueError('turning_demand: share holds one finite weight >= 0 per route (%d)' % R)
    G = int(generations)
    if G < 1:
        raise ValueError('turning_demand: generations must be >= 1')
    if R == 0 or (route_of_agent < 0).any() or (route_of_agent >= R).any():
        raise ValueError('turning_demand: route_of_agent indexes the %d routes' % R)
    routes = [np.asarray(r, dtype=np.float64) for r in routes]
    rng = np.random.default_rng(seed)
    B, A = route_of_agent.shape
    out = np.zeros((B, A, G), dtype=np.int64)
    for b in range(B):
        for a in range(A):
            own, s = int(route_of_agent[b, a]), int(start_index[b, a])
            if not 0 <= s < len(routes[own]):
                raise ValueError('turning_demand: slot (%d, %d) starts at index %d of route %d, which has %d points' % (b, a, s, own, len(routes[own])))
            pose = routes[own][s, :3].tobytes()
            cand = [k for k in range(R) if s < len(routes[k]) and routes[k][s, :3].tobytes() == pose]
            if len(cand) == 1:
                out[b, a, :] = cand[0]
                continue
            w = share[cand]
            if not w.sum() > 0:
                raise ValueError('turning_demand: the candidate routes %s of slot (%d, %d) all have share 0' % (cand, b, a))
            out[b, a, :] = np.asarray(cand)[rng.choice(len(cand), size=G, p=w / w.sum())]
    return out


def stock_routes(ctx: Context, pairs=((1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2))):
    """Reference paths of the stock 4-way intersection, planned with the GPU-backed MotionPrimitiveSearch
    (the `_modified` variant every stock MPC scenario uses); yaw columns unwrapped as MPC.__init__ does."""
    from .lib import _session
    from .lib.car_dimensions import BicycleModelDimensions
    from .lib.motion_primitive import load_motion_primitives
    from .lib.motion_primitive_search import plan_many
    from .lib.motion_primitive_search_modified import MotionPrimitiveSearch
    from .lib.mpc import smooth_yaw
    from .lib.scenario import intersection
    _session.set_context(ctx)
    cd = BicycleModelDimensions()
    mps = load_motion_primitives('bicycle_model')
    routes = []
    searches = [MotionPrimitiveSearch(intersection(start_pos=sp, turn_indicator=ti), cd, mps, margin=cd.radius, ctx=ctx) for sp, ti in pairs]
    for _, _, traj in plan_many(searches):           # all routes planned concurrently (one expansion launch per level)
        traj = np.ascontiguousarray(traj)
        smooth_yaw(traj[:, 2])
        routes.append(traj)
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    return routes, dl, cd


def synthetic_batch(ctx: Context, B: int, A: int = 8, T: int = 20, seed: int = 0, routes=None, dl=None, cd=None,
                    max_start_frac: float = 0.35, instance_slice: Optional[tuple] = None, agent_shard: Optional[tuple] = None,
                    exchange=None, mpc: Optional[MpcParams] = None, stop_mode: str = 'cut', v_ref: Optional[float] = None, route_speed=None):
    """B instances x A agents on the stock intersection, one agent per (arm, manoeuvre)
    route, start positions staggered along the approach (seeded), v0 = 0 as in the reference's scripts.
    The workload is a function of (B, A, seed) only; a rank takes its part of it with instance_slice = (lo, hi)
    (instance-sharded) or agent_shard = (rank, world) (agent-sharded, see IntersectionBatch).
    `mpc` replaces the stock controller constants (its T wins over the argument; the wheelbase is always the car's), e.g.
    MpcParams.jerk() for the controller of lib/mpc_jerk.py.  stop_mode, v_ref, route_speed: see IntersectionBatch."""
    if routes is None:
        routes, dl, cd = stock_routes(ctx)
    rng = np.random.default_rng(seed)
    R = len(routes)
    route_of_agent = np.tile(np.arange(A) % R, (B, 1))
    lens = np.array([len(r) for r in routes])[route_of_agent]
    start = (rng.random((B, A)) * max_start_frac * lens).astype(np.int64)
    if instance_slice is not None:
        lo, hi = instance_slice
        route_of_agent, start = route_of_agent[lo:hi], start[lo:hi]
    if mpc is None:
        params = MpcParams(T=T, L=cd.distance_back_to_front_wheel)
    else:
        params = dataclasses.replace(mpc, L=cd.distance_back_to_front_wheel)
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(ctx, params, ip, routes, dl, route_of_agent, start, agent_shard=agent_shard, exchange=exchange,
                             stop_mode=stop_mode, v_ref=v_ref, route_speed=route_speed)


def scripted_traffic_specs(B: int, K: int, seed: int, L: float, dt: float = 0.2):
    """the scripted cars of scripted_traffic_batch as a runtime.Traffic (host tables only, no GPU needed): K
    MovingObstacleTIntersection per instance, direction +-1, turning or not, speed ~ U[15, 35] / 3.6 m/s, start delay ~ U[0, 6] s,
    drawn with numpy.random.default_rng([seed, 1]); instance 0 carries the stock pair of scenarios/mpc_intersection.py:42-45 in its
    first two places (direction 1, offset 2, straight on / direction -1, offset 4, turning; 25 / 3.6 m/s)."""
    from .lib.moving_obstacles import calculate_steering_angle_for_radius
    rng = np.random.default_rng([seed, 1])
    direction = np.where(rng.random((B, K)) < 0.5, 1, -1)
    turning = rng.random((B, K)) < 0.5
    speed = rng.uniform(15.0, 35.0, (B, K)) / 3.6
    offset = rng.uniform(0.0, 6.0, (B, K))
    if B and K:
        stock = [(1, False, 25 / 3.6, 2.0), (-1, True, 25 / 3.6, 4.0)][:K]
        for k, (d, t, v, o) in enumerate(stock):
            direction[0, k], turning[0, k], speed[0, k], offset[0, k] = d, t, v, o
    actors = np.zeros(B * K, _lib.TRAFFIC_ACTOR_DTYPE)
    d = direction.reshape(-1)
    actors['kind'] = _lib.TRAFFIC_TINTERSECTION
    actors['direction'], actors['turning'] = d, turning.reshape(-1)
    actors['speed'], actors['offset'] = speed.reshape(-1), offset.reshape(-1)
    actors['counter_dt'] = actors['model_dt'] = dt
    actors['L'] = L
    actors['x_turn'] = np.where(d == 1, -10.0, 12.0)
    actors['arc'] = float(calculate_steering_angle_for_radius(5))
    state = np.zeros((B * K, 4))
    state[:, 0], state[:, 1], state[:, 2] = np.where(d == 1, -30.0, 30.0), np.where(d == 1, -3.0, 3.0), np.where(d == 1, 0.0, np.pi)
    return Traffic(actors, state, np.full(B, K, dtype=np.int64))


def scripted_traffic_layout(B: int, A: int, route_lens, seed: int, max_start_frac: float = 0.35, stock_route: int = 6):
    """the egos of scripted_traffic_batch (host arrays only, no GPU needed): (route_of_agent, start_index), both (B, A), drawn with
    numpy.random.default_rng([seed, 0]) for routes of route_lens points; instance 0 is the stock set"""
    R = len(route_lens)
    rng = np.random.default_rng([seed, 0])
    first = rng.integers(0, R, size=B)
    if B:
        first[0] = min(stock_route, R - 1)
    a = np.arange(A)
    route_of_agent = (first[:, None] + 2 * a[None, :] + (2 * a[None, :]) // R) % R        # the next arm first, then the other manoeuvre
    lens = np.asarray(route_lens)[route_of_agent]
    start = (rng.random((B, A)) * max_start_frac * lens).astype(np.int64)
    if B:
        start[0, 0] = 0
    return route_of_agent, start


def scripted_traffic_batch(ctx: Context, B: int, T: int = 20, seed: int = 0, A: int = 1, K: int = 2, routes=None, dl=None, cd=None,
                           max_start_frac: float = 0.35, instance_slice: Optional[tuple] = None, mpc: Optional[MpcParams] = None,
                           stock_route: int = 6, stop_mode: str = 'cut', v_ref: Optional[float] = None, route_speed=None):
    """The reference's stock scenario (scenarios/mpc_intersection.py: one ego + two scripted cars that never yield) as a seeded family of
    B instances: the ego's route uniform over the stock routes, A - 1 further egos on the other arms (every ego yields to every other, as
    in synthetic_batch: start positions staggered along the approach, v0 = 0), K scripted T-intersection cars per instance
    (scripted_traffic_specs).  Instance 0 is ALWAYS the stock set: route `stock_route` of `routes` ((4, 1) of stock_routes), started at
    the first path point, with the stock pair of cars.  A function of (B, seed) only (for given A, K), so a rank takes its part with
    instance_slice = (lo, hi).  stop_mode, v_ref, route_speed: see IntersectionBatch -- with stop_mode='speed' and
    mpc=lib.mpc_with_speed.params(cd, 0.2) the family of the reference's newer script, scenarios/mpc_intersection_new_ref.py."""
    if routes is None:
        routes, dl, cd = stock_routes(ctx)
    route_of_agent, start = scripted_traffic_layout(B, A, [len(r) for r in routes], seed, max_start_frac, stock_route)
    params = MpcParams(T=T, L=cd.distance_back_to_front_wheel) if mpc is None else dataclasses.replace(mpc, L=cd.distance_back_to_front_wheel)
    traffic = scripted_traffic_specs(B, K, seed, cd.distance_back_to_front_wheel, dt=params.dt)
    if instance_slice is not None:
        lo, hi = instance_slice
        route_of_agent, start, traffic = route_of_agent[lo:hi], start[lo:hi], traffic.slice(lo, hi)
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(ctx, params, ip, routes, dl, route_of_agent, start, traffic=traffic, stop_mode=stop_mode, v_ref=v_ref,
                             route_speed=route_speed)


_PLAN_CACHE = {}
ALL_STOCK_PAIRS = tuple((sp, ti) for sp in (1, 2, 3, 4) for ti in (1, 2, 3))


def config2_batch(ctx: Context, B: int = 256, T: int = 20, seed: int = 0, routes=None, dl=None, cd=None, burn_in: int = 3,
                  instance_slice: Optional[tuple] = None, mpc: Optional[MpcParams] = None):
    """SURVEY section 8(d) config 2 (BASELINE configs[1]): B INDEPENDENT single-ego instances (no other agent, hence no coupling), drawn
    with numpy.random.default_rng(seed): route uniform over the 12 stock A* paths (start_pos 1..4 x turn_indicator 1..3), arc position
    s ~ U[0, len - T vmax dt / dl] path points, lateral offset ~ N(0, 0.3 m), heading error ~ N(0, 0.05 rad), v ~ U[0, 30/3.6 m/s];
    `burn_in` (3) closed-loop steps are taken here so that every later step starts from the previous solution -- the generator
    whose QPs have "realistic active sets" (acceleration bound when slow, steering-rate bound in the turns; lib/mpc.py:184-191).
    `routes` must be the 12 paths of stock_routes(ctx, ALL_STOCK_PAIRS) when given.  The workload is a function of (B, T, seed) only;
    instance_slice = (lo, hi) takes a rank's part of it."""
    if routes is None:
        routes, dl, cd = stock_routes(ctx, ALL_STOCK_PAIRS)
    if len(routes) != len(ALL_STOCK_PAIRS):
        raise ValueError('config2_batch draws from the %d stock routes, got %d' % (len(ALL_STOCK_PAIRS), len(routes)))
    params = MpcParams(T=T, L=cd.distance_back_to_front_wheel) if mpc is None else dataclasses.replace(mpc, L=cd.distance_back_to_front_wheel)
    rng = np.random.default_rng(seed)
    route = rng.integers(0, len(routes), size=B)
    lens = np.array([len(r) for r in routes])[route]
    span = np.maximum(lens - params.T * params.max_speed * params.dt / dl, 1.0)
    start = np.floor(rng.random(B) * span).astype(np.int64)
    lateral = rng.normal(0.0, 0.3, B)
    heading = rng.normal(0.0, 0.05, B)
    v0 = rng.uniform(0.0, params.max_speed, B)
    if instance_slice is not None:
        lo, hi = instance_slice
        route, start, lateral, heading, v0 = route[lo:hi], start[lo:hi], lateral[lo:hi], heading[lo:hi], v0[lo:hi]
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    sim = IntersectionBatch(ctx, params, ip, routes, dl, route[:, None], start[:, None], v0=v0[:, None],
                            pose_offset=np.stack([lateral, heading], axis=1)[:, None, :])
    if burn_in > 0:
        sim.run(burn_in)
    return sim


def prius_frontier(ctx: Context, n: int = 1 << 20, seed: int = 0, extent: float = 40.0, free_space: bool = True, embed=None):
    """the search model of the Prius primitives + PriusDimensions on the stock intersection and a
    frontier of n nodes (seeded) as a device tensor.
    free_space = True (the frontier section 8(d) defines): nodes "sampled from free space with theta ~ U[-pi, pi)" -- x, y uniform over
    the junction area, REJECTING every pose at which the car itself collides (one of its two discs inside an obstacle inflated by
    the disc radius: exactly the test check_collision makes on a pose, obstacles.py:157-176), so that no record leaves at a first hit
    that the pose alone decides -- "plus all nodes of the golden expansion logs" (`embed`: (m, 3) array written over the first m
    nodes; bench.py passes the Prius logs of tests/golden/astar_runs.npz).
    free_space = False: round 2's frontier, x, y uniform over the junction area whatever stands there (60 % of its records collide)."""
    from .lib.car_dimensions import PriusDimensions
    from .lib.motion_primitive import load_motion_primitives
    from .lib.motion_primitive_search_modified import MotionPrimitiveSearch
    from .lib.scenario import intersection
    cd = PriusDimensions()
    search = MotionPrimitiveSearch(intersection(start_pos=2, turn_indicator=1), cd, load_motion_primitives('prius'), margin=cd.radius, ctx=ctx)
    rng = np.random.default_rng(seed)

    def draw(m):
        return np.column_stack([rng.uniform(-extent, extent, m), rng.uniform(-extent, extent, m), rng.uniform(-np.pi, np.pi, m)])
    if not free_space:
        nodes = draw(n)
    else:
        hps = search._obstacles_hp                      # per obstacle: rows (a, b, c), inside <=> a x + b y + c <= 0 for every row
        centers = np.asarray(cd.circle_centers, dtype=np.float64)
        parts, have = [], 0
        while have < n:
            cand = draw(max(1 << 16, int(1.6 * (n - have))))
            c, s = np.cos(cand[:, 2]), np.sin(cand[:, 2])
            free = np.ones(len(cand), bool)
            for ox, oy in centers:                      # disc centres of the car at the pose
                px, py = cand[:, 0] + c * ox - s * oy, cand[:, 1] + s * ox + c * oy
                for hp in hps:
                    free &= ~((hp[:, 0][None, :] * px[:, None] + hp[:, 1][None, :] * py[:, None] + hp[:, 2][None, :]) <= 0.0).all(axis=1)
            parts.append(cand[free]); have += int(free.sum())
        nodes = np.concatenate(parts)[:n]
    if embed is not None and len(embed):
        e = np.asarray(embed, dtype=np.float64).reshape(-1, 3)[:n]
        nodes[:len(e)] = e
    return search._model, ctx.f64(nodes)
