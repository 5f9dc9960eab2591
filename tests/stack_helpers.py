"""The whole stack of the device closed loop on the CPU oracle, one step at a time and snapshot to snapshot: stack_step(cfg, words) maps the
words of a batch before a step to the words after it with every optional stage that `cfg` switches on -- admission, the entry-order stamp,
right of way, shared plans, a fixed signal plan or a reservation manager, car following, the advised speed, one or two linearisation passes,
the run log's outcome words, retirement with departure and respawn with routes.  It is composed from the pieces the rule-specific helper
modules already have and takes nothing from the kernels; StackOracleLoop iterates it from a scene description built without a GPU.

The order of a step is enqueue_step's (csrc/mpcx_loop.hip:293-360) and, in its middle, enqueue_search_and_solve's (:224-283):

  head    admission (the host build of mpcx_admit_core.h), then the entry-order stamp (the host build of mpcx_precedence_core.h)
  pool    every row packed from the state and the controls of the step before
  view    what a driving agent sees of a PRESENT row r of its window (absent rows are left out) -- the precedence that the PREC
          instantiation of first_row implements (csrc/mpcx_interaction_parts.h:203-212: the candidate's address is selected between the
          standing records and the predicted frames by the `yields` bit alone, and yielding_rows, :757-763, sets that bit for prec[r] >
          prec[own]; the intent stage has written a sharing row's predicted frames before, mpcx_loop.hip:313-318, and never its standing record):
            1. prec[r] > prec[own]: the standing trajectory (x, y, 0, yaw, 0, 0) rolled out (precedence_helpers.standing)
            2. else, if r is the own row of an agent that shares, drives, is present and whose last status is 0: its plan of the step
               before re-rolled (intent_helpers.seen_trajectory)
            3. else the constant prediction
  search  the conflict search of every driving agent (intent_helpers.intent_search)
  hold    none, the fixed plan (signal_helpers.rule_numpy: the clock, the light, the amber hysteresis) or the reservation manager (the
          host build of mpcx_reserve_core.h on the words of all junctions: a manager decides for all its agents at once)
  follow  on the RAW pool rows (follow_helpers.leader_of / stop_and_cap): the leader's true speed, whoever yields or shares
  advice  advise_helpers.advised_speed on the cut both left (speed mode)
  solve   lin_passes x (window, rollout, QP) with the follower's cap and the advice on every window (intent_helpers.intent_solve)
  tail    the plant; the run log's outcome words (the host build of mpcx_record_core.h); retirement and departure (the host build of
          mpcx_retire_core.h); respawn with routes (the host build of mpcx_route_core.h)

The words are those of IntersectionBatch.snapshot() (`u`, `x`, `cut_len`, `held`, `granted`, `precedence`, ...) and the device words a
snapshot leaves out (`tick`, `clock`, `junction_clock`, `queued`, `path_off`, `path_len`, `prev_len`, `ep_i32`, `ep_f64` and the log's `log_steps`,
`goal_step`, `contact_step`, `flags`, `min_clearance`); in speed mode `cut_len` holds the device's convention, the path length where nothing stops the agent."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

from oracle import oracle_py as orc
from tests import admit_helpers as AH
from tests import advise_helpers as AD
from tests import follow_helpers as FH
from tests import helpers as H
from tests import intent_helpers as IH
from tests import precedence_helpers as PH
from tests import reserve_helpers as RV
from tests import route_helpers as TH
from tests import scene_helpers as SH
from tests import signal_helpers as G
from tests import speedref_helpers as S

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE_SRC = os.path.join(HERE, 'scene_ref', 'scene_ref.cpp')
STOCK_PAIRS = IH.STOCK_PAIRS
PRED_STEPS, FRAME_WINDOW, MAX_ACCEL = 35, 20, 2.0

# the integer words a step must reproduce exactly, the floats it must reproduce bit for bit, and the ones it reproduces within a bound
INT_WORDS = ('traj_idx', 'cut_len', 'prev_len', 'target_ind', 'hit_idx', 'status', 'held', 'leader', 'done', 'steps_driven', 'absent', 'wait',
             'entered_step', 'clock', 'served', 'path_off', 'path_len', 'precedence', 'granted', 'since', 'occupied', 'queued', 'junction_clock',
             'shared_frames', 'tick', 'ep_i32', 'log_steps', 'goal_step', 'contact_step', 'flags')
BIT_WORDS = ('gap', 'follow_cap', 'advised')
NEAR_WORDS = ('u', 'x', 'state', 'applied')         # within TOL
CLEAR_WORDS = ('min_clearance', 'ep_f64')           # within CLEAR_TOL
TOL = 2e-7              # the project's bar in every closed-loop replay
# the bound tests/test_gpu_scene.py puts on the device's clearance against its restatement (the same disc centres through another sincos)
CLEAR_TOL = 1e-12
EVENTS = ('new_route', 'ended_held', 'ended_leading', 'ended_granted', 'leader_yields', 'leader_shares', 'follow_cut_while_held',
          'hold_cut_with_leader', 'stand_and_plan', 'cap_lowered', 'advice_lowered', 'refused_by_grant', 'granted', 'episodes')


# ---------------------------------------------------------------- the host builds
def build_libs(directory):
    """the host builds a step goes through, compiled as the rule-specific helpers compile them (g++ -ffp-contract=off)"""
    from mpc_for_av_at_intersection_amd import _lib
    d = str(directory)
    so = os.path.join(d, 'libscene_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + AH.INC + ['-o', so, SCENE_SRC], check=True)
    scene = C.CDLL(so)
    scene.scene_ref_record_step.restype = None
    scene.scene_ref_record_step.argtypes = ([C.POINTER(_lib.InteractionParamsC), C.c_int, C.c_int] + [C.c_void_p] * 12 + [C.c_int] + [C.c_void_p] * 4 +
                                            [C.POINTER(_lib.RunLogC)] + [C.c_void_p] * 3)
    scene.scene_ref_retire_step.restype = C.c_int
    scene.scene_ref_retire_step.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.POINTER(_lib.RetireC), C.POINTER(_lib.SceneC), C.c_void_p]
    return types.SimpleNamespace(admit=AH.build_ref(d), stamp=PH.build_ref(d), reserve=RV.build_ref(d), route=TH.build_ref(d), scene=scene)


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


# ---------------------------------------------------------------- what is switched on
def make_config(libs, routes, dl, B, A, T=13, speed=False, retire=True, gap=None, due=None, route_of=None, start_idx=None, log=False,
                precedence=None, signals=None, reserve=None, advice=None, share=None, follow=None, lin_passes=1, v_ref=S.V_REF):
    """The description of a batch of B instances x A agents on `routes` (a list of (n, 3) paths; the pool is [A agents] per instance):
    retire: retirement with departure; gap, due, route_of, start_idx ((B, A, G) each): admission and respawn with routes; log: the run
    log's outcome words; precedence: None, 'entry' or 'fixed'; signals: dict(plans, plan_of (P,), stop, group, brake) with the tables per
    path point; reserve: dict(managers [(detect, patience)], mgr_of (B,), stop, group, exit, conflict, lane); advice: dict(v_cruise, v_min,
    reach, lead); share: (P,) flags; follow: dict(standstill, time_gap, brake, v_min, lateral, heading, reach)."""
    cd = SH.car()
    P = B * A
    c = types.SimpleNamespace(libs=libs, B=B, A=A, P=P, T=T, speed=bool(speed), dl=float(dl), v_ref=float(v_ref), lin_passes=int(lin_passes))
    c.p = S.speed_params(T=T, L=cd.distance_back_to_front_wheel) if speed else orc.MpcParams(T=T, L=cd.distance_back_to_front_wheel)
    c.centers, c.radius = np.asarray(cd.circle_centers, dtype=np.float64).reshape(2, 2), float(cd.radius)
    c.margin = 4 * int(np.ceil(cd.radius / dl))
    c.pred_steps, c.frame_window, c.max_accel = PRED_STEPS, FRAME_WINDOW, MAX_ACCEL
    c.routes = [np.ascontiguousarray(r, dtype=np.float64) for r in routes]
    lens = np.array([len(r) for r in c.routes])
    c.path = np.concatenate(c.routes)
    c.route_off, c.route_len = _i32(np.cumsum(np.concatenate([[0], lens[:-1]]))), _i32(lens)
    c.obs_off, c.obs_cnt, c.obs_skip = _i32(np.repeat(np.arange(B) * A, A)), _i32(np.full(P, A)), _i32(np.arange(P))
    c.retire, c.log, c.precedence = bool(retire), bool(log), precedence
    c.goal_dis, c.stop_speed = SH.GOAL_DIS, SH.STOP_SPEED
    c.gap = None if gap is None else float(gap)
    c.respawn = None
    if due is not None:
        due, route_of, start_idx = (_i32(v).reshape(P, -1) for v in (due, route_of, start_idx))
        G_ = due.shape[1]
        rs = np.zeros((P, G_, 4))
        pts = c.path[c.route_off[route_of] + start_idx]
        rs[..., 0], rs[..., 1], rs[..., 3] = pts[..., 0], pts[..., 1], pts[..., 2]
        c.respawn = dict(G=G_, due=due, route_of=route_of, rstart_idx=start_idx, rstart_state=rs, start_state=rs[:, 0].copy(), start_idx=start_idx[:, 0].copy())
    c.signals = None
    if signals is not None:
        c.signals = dict(path_stop=_i32(signals['stop']), path_group=_i32(signals['group']), plan_cycle=_i32([pl['cycle'] for pl in signals['plans']]),
                         plan_amber=_i32([pl['amber'] for pl in signals['plans']]), plan_green=_i32(np.stack([pl['green'] for pl in signals['plans']])),
                         plan_of=_i32(signals.get('plan_of', np.zeros(P))), brake=float(signals.get('brake', abs(c.p.max_decel))))
    c.reserve = None
    if reserve is not None:
        big = RV.UNBOUNDED
        c.reserve = dict(path_stop=_i32(reserve['stop']), path_group=_i32(reserve['group']), path_exit=_i32(reserve['exit']),
                         conflict=_i32(reserve['conflict']), lane=_i32(reserve['lane']),
                         mgr_time=_i32([[d, big if pt is None else pt] for d, pt in reserve['managers']]), mgr_of=_i32(reserve.get('mgr_of', np.zeros(B))),
                         brake=float(reserve.get('brake', abs(c.p.max_decel))), n_groups=len(reserve['conflict']))
    c.advice = None if advice is None else dict(advice)
    c.share = None if share is None else _i32(np.asarray(share) != 0)
    c.follow = None if follow is None else dict(follow)
    return c


def initial_words(cfg, route, start, tick=None, prec=None):
    """the words of a fresh batch: agents on routes `route` (P,) from the indices `start` (P,), v0 = 0; with respawn the first vehicles'
    routes and indices, everybody waiting at the gate (IntersectionBatch.respawn_on_schedule).  tick: the signal clocks (P,); prec: fixed words"""
    P, T = cfg.P, cfg.T
    if cfg.respawn is not None:
        route, start = cfg.respawn['route_of'][:, 0], cfg.respawn['rstart_idx'][:, 0]
    route, start = _i32(route).reshape(P), _i32(start).reshape(P)
    pts = cfg.path[cfg.route_off[route] + start]
    w = dict(state=np.column_stack([pts[:, 0], pts[:, 1], np.zeros(P), pts[:, 2]]), applied=np.zeros((P, 2)), traj_idx=start.copy(),
             target_ind=start.copy(), cut_len=np.zeros(P, np.int32), prev_len=np.zeros(P, np.int32), u=np.zeros((P, 2, T)), x=np.zeros((P, 4, T + 1)),
             xref=np.zeros((P, 4, T + 1)), status=np.zeros(P, np.int32), hit_idx=np.zeros(P, np.int32), iters=np.zeros(P, np.int32),
             path_off=cfg.route_off[route].copy(), path_len=cfg.route_len[route].copy(), done=np.zeros(P, np.int32), steps_driven=np.zeros(P, np.int32),
             absent=np.zeros(P, np.int32))
    if cfg.gap is not None:
        wait = cfg.respawn['due'][:, 0].copy()
        w.update(wait=wait, entered_step=_i32(np.where(wait >= 0, -1, 0)), clock=np.zeros(1, np.int32))
        w['done'][wait >= 0] = 1
        w['absent'][cfg.obs_skip[wait >= 0]] = 1
    if cfg.respawn is not None:
        G_ = cfg.respawn['G']
        w.update(served=np.zeros(P, np.int32), ep_i32=np.zeros((P, G_, 8), np.int32), ep_f64=np.zeros((P, G_, 2)))
    if cfg.log:
        w.update(log_steps=np.zeros(P, np.int32), goal_step=np.full(P, -1, np.int32), contact_step=np.full(P, -1, np.int32), flags=np.zeros(P, np.int32),
                 min_clearance=np.full(P, np.inf))
    if cfg.precedence is not None:
        w['precedence'] = np.zeros(P, np.int32) if prec is None else _i32(prec).reshape(P)
    if cfg.signals is not None:
        w.update(tick=np.zeros(P, np.int32) if tick is None else _i32(tick).reshape(P), held=np.zeros(P, np.int32))
    if cfg.reserve is not None:
        w.update(held=np.zeros(P, np.int32), granted=np.zeros(P, np.int32), since=np.full(P, -1, np.int32), junction_clock=np.zeros(cfg.B, np.int32),
                 occupied=np.zeros(cfg.B, np.int32), queued=np.zeros(cfg.B, np.int32))
    if cfg.advice is not None:
        w['advised'] = np.zeros(P)
    if cfg.share is not None:
        w['shared_frames'] = np.zeros(P, np.int32)
    if cfg.follow is not None:
        w.update(leader=np.full(P, -1, np.int32), gap=np.full(P, -1.0), follow_cap=np.zeros(P))
    return w


# ---------------------------------------------------------------- one step
def _ip(cfg):
    return AH.interaction_params(cfg.radius, cfg.centers.ravel())


def _admit(cfg, w):
    case = AH.Case(w['state'], own=cfg.obs_skip, wait=w['wait'], done=w['done'], absent=w['absent'], gap=cfg.gap, radius=cfg.radius,
                   centers=cfg.centers.ravel(), obs_off=cfg.obs_off, obs_cnt=cfg.obs_cnt, clock=int(w['clock'][0]), entered=w['entered_step'])
    AH.host_step(cfg.libs.admit, case)
    w.update(done=case.done, absent=case.absent, wait=case.wait, entered_step=case.entered, clock=case.clock)


def _record(cfg, w, pool, done, absent):
    from mpc_for_av_at_intersection_amd import _lib
    P = cfg.P
    log = _lib.RunLogC()
    log.capacity, log.goal_dis, log.stop_speed = 0, cfg.goal_dis, cfg.stop_speed
    scratch = (np.zeros((1, P, 8)), np.zeros((1, P, 8), np.int32))
    log.rows_f64, log.rows_i32 = scratch[0].ctypes.data, scratch[1].ctypes.data
    for n, k in (('steps', 'log_steps'), ('goal_step', 'goal_step'), ('contact_step', 'contact_step'), ('flags', 'flags'), ('min_clearance', 'min_clearance')):
        setattr(log, n, w[k].ctypes.data)
    ip = _ip(cfg)
    keep = [_f64(w['state']), _f64(w['applied']), _f64(w['x']), cfg.path, _i32(w['path_off']), _i32(w['path_len']), _i32(w['target_ind']),
            _i32(w['cut_len']), _i32(w['traj_idx']), _i32(w['hit_idx']), _i32(w['status']), _i32(w['iters'])]
    tail = [_f64(pool), cfg.obs_off, cfg.obs_cnt, cfg.obs_skip]
    goal_len = _i32(w['path_len']) if cfg.speed else None
    cfg.libs.scene.scene_ref_record_step(C.byref(ip), P, cfg.T, *[a.ctypes.data for a in keep], len(pool), *[a.ctypes.data for a in tail], C.byref(log),
                                         None if goal_len is None else goal_len.ctypes.data, done.ctypes.data, absent.ctypes.data)


def _retire(cfg, w):
    from mpc_for_av_at_intersection_amd import _lib
    r = _lib.RetireC(w['done'].ctypes.data, w['steps_driven'].ctypes.data, cfg.goal_dis, cfg.stop_speed)
    sc = _lib.SceneC(w['absent'].ctypes.data, len(w['absent']), 0)
    goal_len = _i32(w['path_len'] if cfg.speed else w['cut_len'])
    keep = [_i32(w['path_off']), _i32(w['path_len']), _i32(w['target_ind'])]
    return cfg.libs.scene.scene_ref_retire_step(cfg.P, w['state'].ctypes.data, w['applied'].ctypes.data, cfg.path.ctypes.data, *[a.ctypes.data for a in keep],
                                                goal_len.ctypes.data, C.byref(r), C.byref(sc), cfg.obs_skip.ctypes.data)


def _respawn(cfg, w):
    P, T, rs = cfg.P, cfg.T, cfg.respawn
    logw = {}
    if cfg.log:
        logw = dict(lsteps=w['log_steps'], goal_step=w['goal_step'], contact_step=w['contact_step'], flags=w['flags'], min_clearance=w['min_clearance'])
    case = TH.Case(P, T, rs['G'], P, len(cfg.routes), log=cfg.log, speed=cfg.speed, state=w['state'], applied=w['applied'], u=w['u'].reshape(P, 2 * T),
                   start_state=rs['start_state'], traj_idx=w['traj_idx'], target_ind=w['target_ind'], cut_len=w['cut_len'],
                   prev_len=w['prev_len'] if cfg.speed else np.zeros(P), iters=w['iters'], own=cfg.obs_skip, done=w['done'], steps_driven=w['steps_driven'], wait=w['wait'], entered=w['entered_step'],
                   clock=w['clock'], start_idx=rs['start_idx'], due=rs['due'], served=w['served'], ep_i32=w['ep_i32'], ep_f64=w['ep_f64'],
                   route_off=cfg.route_off, route_len=cfg.route_len, route_of=rs['route_of'], rstart_idx=rs['rstart_idx'], rstart_state=rs['rstart_state'],
                   path_off=w['path_off'], path_len=w['path_len'], **logw)
    n = TH.host_step(cfg.libs.route, case)
    w.update(state=case.state, applied=case.applied, u=case.u.reshape(P, 2, T), traj_idx=case.traj_idx, target_ind=case.target_ind, cut_len=case.cut_len,
             iters=case.iters, steps_driven=case.steps_driven, wait=case.wait, entered_step=case.entered, served=case.served, ep_i32=case.ep_i32,
             ep_f64=case.ep_f64, path_off=case.path_off, path_len=case.path_len)
    if cfg.speed:
        w['prev_len'] = case.prev_len
    if cfg.log:
        w.update(log_steps=case.lsteps, goal_step=case.goal_step, contact_step=case.contact_step, flags=case.flags, min_clearance=case.min_clearance)
    return n


def stack_step(cfg, before):
    """One step of the whole stack: the words after it from the words before it (neither is modified), and what happened in it:
    (after, info) with info = dict(events={name: count}, agents={q: dict(...)}, admitted=[...], arrived=[...]).  See the module's docstring
    for the order of the step and for what an agent sees of a row."""
    P, T, speed, p = cfg.P, cfg.T, cfg.speed, cfg.p
    w = {k: np.array(v, copy=True) for k, v in before.items()}
    ev = dict.fromkeys(EVENTS, 0)
    own = cfg.obs_skip
    # ---- the head of the step
    done0 = before['done'].copy()
    if cfg.gap is not None:
        _admit(cfg, w)
    admitted = [q for q in range(P) if done0[q] and not w['done'][q]]
    if cfg.precedence == 'entry':
        PH.host_stamp(cfg.libs.stamp, w['precedence'], w['entered_step'], own, cfg.obs_off, P)
    done, absent = w['done'].copy(), w['absent'].copy()         # as every stage of this step reads them
    pool = np.column_stack([before['state'], before['applied'][:, 1], before['applied'][:, 0]])
    drive = [q for q in range(P) if not done[q]]
    # ---- what the others see of a row
    cc = cfg.centers.ravel()
    takes = np.zeros(P, bool)
    if cfg.share is not None:
        takes = np.array([bool(cfg.share[q]) and not done[q] and not absent[own[q]] and before['status'][q] == IH.OPTIMAL for q in range(P)])
        w['shared_frames'] = _i32(np.where(takes, cfg.pred_steps, 0))
    owner = {int(own[q]): q for q in range(P)}
    cache = {}

    def seen(r, how):
        if (r, how) not in cache:
            if how == 'stand':
                cache[r, how] = orc.predict_obstacle(PH.standing(pool[r:r + 1], [0])[0], p.dt, p.L, cfg.pred_steps)
            else:
                plan = (before['state'][owner[r]].copy(), before['u'][owner[r]].copy()) if how == 'plan' else None
                cache[r, how] = IH.seen_trajectory(p, pool[r], plan, cc, cfg.pred_steps)
        return cache[r, how]

    def view_of(q, r):
        if cfg.precedence is not None and w['precedence'][r] > w['precedence'][own[q]]:
            return 'stand'
        return 'plan' if r in owner and takes[owner[r]] else 'const'

    # ---- the conflict search of every driving agent
    agents, views = {}, {}
    for q in drive:
        full = cfg.path[before['path_off'][q]:before['path_off'][q] + before['path_len'][q]]
        window = [r for r in range(cfg.obs_off[q], cfg.obs_off[q] + cfg.obs_cnt[q]) if r != own[q]]
        present = [r for r in window if not absent[r]]
        how = [view_of(q, r) for r in present]
        for r, h in zip(present, how):
            views.setdefault(r, set()).add(h)
        prev = int(before['prev_len'][q] if speed else before['cut_len'][q])
        ti, hit, cut, _ = IH.intent_search(p, full, before['state'][q], [seen(r, h) for r, h in zip(present, how)], int(before['traj_idx'][q]), prev,
                                           cfg.centers, cfg.radius, cfg.margin, speed, cfg.frame_window, cfg.max_accel)
        if hit is None:
            cut = len(full)             # (speed mode: the device keeps the path length for "no stop", which zeroes nothing)
        agents[q] = dict(full=full, present=present, how=how, conflict_cut=int(cut))
        w['traj_idx'][q], w['cut_len'][q], w['hit_idx'][q] = ti, cut, -1 if hit is None else int(hit[2])
    ev['stand_and_plan'] = sum(1 for r, hs in views.items() if 'stand' in hs and 'plan' in hs)
    # ---- the hold
    line = np.full(P, -1)
    if cfg.reserve is not None:
        tabs = {k: cfg.reserve[k] for k in ('path_stop', 'path_group', 'path_exit', 'conflict', 'lane', 'mgr_time', 'mgr_of', 'brake', 'n_groups')}
        rw = RV.words(state=before['state'], path_off=before['path_off'], path_len=before['path_len'], traj_idx=w['traj_idx'], cut_len=w['cut_len'],
                      done=done, held=w['held'], grant=w['granted'], since=w['since'], clock=w['junction_clock'], occupied=w['occupied'],
                      queued=w['queued'], dl=cfg.dl, n_per=cfg.A, **tabs)
        rn = RV.copy_words(rw)
        RV.host_rule(cfg.libs.reserve, rw)
        grants, refused = [], []
        RV.rule_numpy(rn, log=grants, refused=refused)           # the restated rule, for what happened and why
        for k in RV.OUT_KEYS:
            assert rn[k].tobytes() == rw[k].tobytes(), k
        w.update(held=rw['held'], granted=rw['grant'], since=rw['since'], junction_clock=rw['clock'], occupied=rw['occupied'], queued=rw['queued'],
                 cut_len=rw['cut_len'])
        ev['granted'] = len(grants)
        ev['refused_by_grant'] = sum(1 for _, _, g, occ, _, _ in refused if int(tabs['conflict'][g]) & occ)
        for q in drive:
            if w['held'][q]:
                line[q] = RV.classify(rw, q)[2] + int(w['traj_idx'][q])
    elif cfg.signals is not None:
        tabs = {k: cfg.signals[k] for k in ('path_stop', 'path_group', 'plan_cycle', 'plan_amber', 'plan_green', 'plan_of', 'brake')}
        sw = G.words(state=before['state'], path_off=before['path_off'], path_len=before['path_len'], traj_idx=w['traj_idx'], cut_len=w['cut_len'],
                     done=done, tick=w['tick'], held=w['held'], dl=cfg.dl, **tabs)
        G.rule_numpy(sw)
        w.update(held=sw['held'], tick=sw['tick'], cut_len=sw['cut_len'])
        for q in drive:
            if w['held'][q]:
                line[q] = int(tabs['path_stop'][int(before['path_off'][q]) + int(w['traj_idx'][q])])
    # ---- following, the advice, the solve
    if cfg.follow is not None:
        w['leader'][:], w['gap'][:], w['follow_cap'][:] = -1, -1.0, 0.0
    if cfg.advice is not None:
        w['advised'][:] = 0.0
    for q in drive:
        a = agents[q]
        full, ti, st = a['full'], int(w['traj_idx'][q]), before['state'][q]
        cut = int(w['cut_len'][q])
        a.update(held=int(w['held'][q]) if 'held' in w else 0, line=int(line[q]), hold_cut=cut, stop=-1)
        caps = []
        if cfg.follow is not None:
            slots = FH.others_of(int(cfg.obs_off[q]), int(cfg.obs_cnt[q]), int(own[q]), P, absent)
            best = FH.leader_of(full, ti, pool, slots, cfg.follow, cfg.follow['reach'])
            if best is not None:
                gap, s, cap = FH.stop_and_cap(ti, best[1], best[2], st[2], cfg.dl, speed, cfg.follow)
                w['leader'][q], w['gap'][q], w['follow_cap'][q] = best[0], gap, cap
                a['stop'] = s
                cut = min(cut, s)
        if cfg.advice is not None and speed:
            sg = cfg.signals
            plan = int(sg['plan_of'][q])
            i = int(before['path_off'][q]) + ti
            if 0 <= plan < len(sg['plan_cycle']) and int(sg['plan_cycle'][plan]) >= 1 and 0 <= i < len(sg['path_stop']):
                s, g = int(sg['path_stop'][i]), int(sg['path_group'][i])
                if not (s < 0 or ti >= s or s >= len(full) or not 0 <= g < sg['plan_green'].shape[1] or cut < s):
                    w['advised'][q] = AD.advised_speed(ti, s, int(w['tick'][q]), int(sg['plan_cycle'][plan]), int(sg['plan_green'][plan, g, 0]),
                                                       int(sg['plan_green'][plan, g, 1]), cfg.dl, p.dt, **cfg.advice)
            caps.append(float(w['advised'][q]))
        if cfg.follow is not None and speed:
            caps.append(float(w['follow_cap'][q]))
        r = IH.intent_solve(p, full, cfg.dl, st, int(before['target_ind'][q]), before['u'][q], cut, speed, v_ref=cfg.v_ref, caps=caps,
                            passes=cfg.lin_passes)
        sol = r['sol']
        assert sol.status == 0, (q, sol.status)
        w['cut_len'][q], w['target_ind'][q], w['status'][q], w['iters'][q] = cut, r['target_ind'], sol.status, sol.iters
        w['u'][q], w['x'][q], w['xref'][q] = sol.u, sol.x, r['xref']
        if speed:
            w['prev_len'][q] = len(full)
        w['state'][q] = orc.plant_step(p, st, sol.u[0, 0], sol.u[1, 0])
        w['applied'][q] = (sol.u[1, 0], sol.u[0, 0])
        # what happened to this agent
        a.update(cut=cut, leader=int(w['leader'][q]) if cfg.follow is not None else -1)
        if a['leader'] >= 0:
            lr = a['leader']
            ev['leader_yields'] += bool(cfg.precedence is not None and w['precedence'][lr] > w['precedence'][own[q]])
            ev['leader_shares'] += bool(lr in owner and takes[owner[lr]])
            if a['held']:
                ev['follow_cut_while_held'] += bool(a['stop'] == cut and a['stop'] < a['line'] and a['stop'] < a['conflict_cut'])
                ev['hold_cut_with_leader'] += bool(a['line'] == cut and a['line'] < a['stop'] and a['line'] < a['conflict_cut'])
        if speed and len(caps):
            free = r['xref_free'][2]
            adv = np.minimum(free, w['advised'][q]) if cfg.advice is not None and w['advised'][q] > 0.0 else free
            ev['advice_lowered'] += bool((adv < free).any())
            ev['cap_lowered'] += bool((r['xref'][2] < adv).any())
    # ---- the tail of the step
    if cfg.log:
        _record(cfg, w, pool, done, absent)
    arrived = []
    if cfg.retire:
        _retire(cfg, w)
        arrived = [q for q in drive if w['done'][q]]
    for q in arrived:
        ev['ended_held'] += bool('held' in w and w['held'][q] != 0)
        ev['ended_leading'] += bool(cfg.follow is not None and (w['leader'] == own[q]).any())
        ev['ended_granted'] += bool('granted' in w and w['granted'][q] != 0)
    if cfg.respawn is not None:
        for q in admitted:
            g = int(before['served'][q])
            ev['new_route'] += bool(g > 0 and cfg.respawn['route_of'][q, g] != cfg.respawn['route_of'][q, g - 1])
        _respawn(cfg, w)
        ev['episodes'] = int((w['served'] - before['served']).sum())
    return w, dict(events=ev, agents=agents, admitted=admitted, arrived=arrived, pool=pool)


def compare_words(got, want, cfg, what=''):
    """`got` (the device's words after a step) against `want` (stack_step's): INT_WORDS identical, BIT_WORDS bit for bit, row 2 of xref
    equal in speed mode for whoever drove, NEAR_WORDS within TOL, CLEAR_WORDS within CLEAR_TOL (infinities equal).  Returns the worst
    |difference| over NEAR_WORDS."""
    for k in INT_WORDS:
        if k in want and k in got:
            assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero((np.asarray(got[k]) != np.asarray(want[k])).reshape(len(want[k]), -1).any(1))[:8],
                                                     np.asarray(got[k]).ravel()[:16], np.asarray(want[k]).ravel()[:16])
    for k in BIT_WORDS:
        if k in want and k in got:
            assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    if cfg.speed:
        assert np.array_equal(got['xref'][:, 2], want['xref'][:, 2]), (what, 'xref', np.flatnonzero((got['xref'][:, 2] != want['xref'][:, 2]).any(1)))
    worst = 0.0
    for k in NEAR_WORDS:
        worst = max(worst, float(np.abs(got[k] - want[k]).max()))
        assert worst < TOL, (what, k, worst)
    for k in CLEAR_WORDS:
        if k in want and k in got:
            fin = np.isfinite(want[k])
            assert np.array_equal(got[k][~fin], want[k][~fin]) and (np.abs(got[k][fin] - want[k][fin]) <= CLEAR_TOL).all(), (what, k)
    return worst


# ---------------------------------------------------------------- the free-running loop
class StackOracleLoop:
    """stack_step iterated from initial_words: the instrument the scenes of tests/test_gpu_stack.py are chosen with"""

    def __init__(self, cfg, words):
        self.cfg, self.words, self.steps = cfg, words, 0
        self.events = dict.fromkeys(EVENTS, 0)
        self.episodes_of = np.zeros(cfg.B, np.int64)
        self.last = None

    def step(self):
        before = self.words
        self.words, self.last = stack_step(self.cfg, before)
        for k, v in self.last['events'].items():
            self.events[k] += int(v)
        if 'served' in self.words:
            self.episodes_of += (self.words['served'] - before['served']).reshape(self.cfg.B, -1).sum(1)
        self.steps += 1
        return self.last

    def run(self, n):
        for _ in range(n):
            self.step()
        return self.events


# ---------------------------------------------------------------- the scenes of tests/test_gpu_stack.py
FOLLOW = dict(standstill=6.0, time_gap=1.0, brake=3.0, v_min=0.5, lateral=1.5, heading=0.8)


def stock_paths():
    paths = [H.smoothed_path(*pr) for pr in STOCK_PAIRS]
    return paths, float(np.linalg.norm(paths[0][0, :2] - paths[0][1, :2]))


def follow_params(dl, **kw):
    """IntersectionBatch.follow's defaults: reach 40 m of path points"""
    return dict(FOLLOW, reach=int(round(40.0 / dl)), **kw)


WIDE = dict(standstill=12.0, time_gap=1.5)      # tests/test_gpu_follow.py: wider than the 10.3 m at which the conflict search stops a follower by itself
PLAN = dict(cycle=60, green=18, amber=5)
B_, A_, G_ = 2, 8, 3


def exit_lines(routes, stop, group, back=3):
    """stop_lines()' tables with a second line per route, `back` points before its last point, for the points behind the first line: a
    signal on the exit arm (same group as the approach).  A car the light holds there stands within the goal distance of its route's end,
    so it can arrive -- and hand its slot on -- while it is held."""
    stop, group = np.array(stop, copy=True), np.array(group, copy=True)
    off = 0
    for r in routes:
        n, s1 = len(r), int(stop[off])
        if s1 >= 0:
            stop[off + s1 + 1:off + n - back + 1] = n - back
            group[off + s1 + 1:off + n - back + 1] = group[off]
        off += n
    return stop, group


def scene(kind, routes):
    """The scene of tests/test_gpu_stack.py K1 (kind 'plan') and K2 ('reserve') as plain arrays, B = 2 instances x A = 8 slots x G = 3
    vehicles: slots 2k and 2k + 1 serve arm k.  The first vehicles stand in line on one route of their arm, 10.8 m apart, 11 to 22 m before
    its end (instance 0: the straight routes, instance 1: the turning ones; the exits of the four arms are distinct); the later ones enter
    at index 0 of the straight or the turning route of the arm, the two slots of an arm from the same pose, so that the gate queues them.
    Returns dict(route_of, start_idx, due, gap, share, offset, follow, ...) with the tables of the kind."""
    from mpc_for_av_at_intersection_amd.batch import movement_conflicts, movement_lines, stop_lines, two_phase_plan
    lens = np.array([len(r) for r in routes])
    route_of, start_idx, due = (np.zeros((B_, A_, G_), np.int64) for _ in range(3))
    for b in range(B_):
        for a in range(A_):
            k, j = a // 2, a % 2
            first, other = 2 * k + (1 - b), 2 * k + b
            route_of[b, a] = [first, other, first] if j == 0 else [first, first, other]
            start_idx[b, a, 0] = lens[first] - (130 if j else 260) - 10 * k
            due[b, a] = [2 * a * b, 24 + 5 * a + 3 * b, 70 + 4 * a + 5 * b]
    share = np.array([[a % 2 == 1 - b for a in range(A_)] for b in range(B_)]).reshape(-1).astype(np.int32)
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    out = dict(route_of=route_of, start_idx=start_idx, due=due, gap=1.0, share=share, follow=dict(follow_params(dl), **WIDE))
    if kind == 'plan':
        stop, group = exit_lines(routes, *stop_lines(routes))
        out.update(plan=two_phase_plan(**PLAN), stop=stop, group=group, offset=np.array([0, 20]))
    else:
        stop, group, ex = movement_lines(routes)
        cd = SH.car()
        conflict, lane = movement_conflicts(routes, stop, ex, np.asarray(cd.circle_centers, dtype=np.float64), float(cd.radius))
        out.update(stop=stop, group=group, exit=ex, conflict=conflict, lane=lane, managers=[(int(stop.max()), 0), (int(stop.max()), None)],
                   mgr_of=np.array([0, 1]))
    return out


def scene_config(libs, kind, speed, routes, dl):
    """(cfg, initial words, scene) of K1 / K2 in cut or speed mode"""
    sc = scene(kind, routes)
    kw = dict(speed=speed, gap=sc['gap'], due=sc['due'], route_of=sc['route_of'], start_idx=sc['start_idx'], log=True, precedence='entry',
              share=sc['share'], follow=sc['follow'])
    if kind == 'plan':
        kw['signals'] = dict(plans=[sc['plan']], stop=sc['stop'], group=sc['group'])
        if speed:
            kw['advice'] = dict(AD.ADVICE)
    else:
        kw['reserve'] = {k: sc[k] for k in ('managers', 'mgr_of', 'stop', 'group', 'exit', 'conflict', 'lane')}
    cfg = make_config(libs, routes, dl, B_, A_, **kw)
    tick = np.repeat(sc['offset'], A_) if kind == 'plan' else None
    return cfg, initial_words(cfg, None, None, tick=tick), sc


# the smallest step counts (to the next multiple of five, the chunk of the graph replay) at which the free run on the CPU has shown every
# event of REQUIRED: the last to appear is an agent whose hold is the shortest cut while it has a leader, in step 108 (K1) and 96 (K2, cut mode)
STEPS = dict(plan=110, reserve=100)
# the events a scene must contain.  Not among them: `ended_granted` -- with the tables of movement_lines() a car gives the crossing back at
# its exit point, 13 m or more before its route's end --, and in speed mode `ended_held`: a car that the light holds at the line on the exit
# arm creeps over it at 0.2 to 0.3 m/s, faster than the goal test's stop speed, and arrives behind the line, free.
COMMON = ('new_route', 'ended_leading', 'leader_yields', 'leader_shares', 'follow_cut_while_held', 'hold_cut_with_leader', 'stand_and_plan', 'episodes')
REQUIRED = {('plan', False): COMMON + ('ended_held',), ('plan', True): COMMON + ('cap_lowered', 'advice_lowered'),
            ('reserve', False): COMMON + ('refused_by_grant', 'granted'), ('reserve', True): COMMON + ('refused_by_grant', 'granted', 'cap_lowered')}

QUEUE_ROUTE, QUEUE_START = 1, np.array([[400, 300, 200, 100], [420, 330, 240, 150]])      # tests/test_gpu_follow.py's queue


def queue_config(libs, routes, dl, lin_passes=2):
    """K4: the queue of tests/test_gpu_follow.py -- 2 x 4 cars in line on the straight route from the south -- in speed mode without signals
    and without retirement, following with the wide gap, two linearisation passes"""
    cfg = make_config(libs, routes, dl, 2, 4, speed=True, retire=False, follow=dict(follow_params(dl), **WIDE), lin_passes=lin_passes)
    return cfg, initial_words(cfg, np.full(8, QUEUE_ROUTE), QUEUE_START.reshape(-1))
