"""ctypes binding of libmpcx.so (the HIP/gfx950 hot path). There is NO CPU fallback: if the library is
missing or no GPU is usable the loaders below raise."""
import ctypes as C
import os
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPCX_LIB: developer override (another build of the same sources, such as the MPCX_INTER_FORCE_EXACT one); the product is libmpcx.so
LIB_PATH = os.environ.get('MPCX_LIB') or os.path.join(_HERE, 'libmpcx.so')
_lib = None

c_dp = C.c_void_p  # device pointers travel as raw addresses


MODEL_BICYCLE4, MODEL_JERK5 = 0, 1      # mpcx_mpc_params.model


class MpcParamsC(C.Structure):
    """mirror of mpcx_mpc_params (include/mpcx.h)"""
    _fields_ = [('T', C.c_int32), ('max_iter', C.c_int32), ('dt', C.c_double), ('L', C.c_double),
                ('w_perp', C.c_double), ('w_para', C.c_double), ('R', C.c_double * 2), ('Rd', C.c_double * 2),
                ('Q_v_yaw', C.c_double * 2), ('Qf', C.c_double * 4), ('R_end', C.c_double * 2),
                ('max_speed', C.c_double), ('min_speed', C.c_double), ('max_accel', C.c_double),
                ('max_decel', C.c_double), ('max_steer', C.c_double), ('max_dsteer', C.c_double), ('tol', C.c_double),
                ('model', C.c_int32), ('reserved', C.c_int32), ('jerk_weight', C.c_double)]


class InteractionParamsC(C.Structure):
    """mirror of mpcx_interaction_params (include/mpcx.h)"""
    _fields_ = [('pred_steps', C.c_int32), ('frame_window', C.c_int32),
                ('cutoff_margin', C.c_int32), ('max_path_len', C.c_int32), ('dt', C.c_double), ('L', C.c_double), ('radius', C.c_double),
                ('circle_centers', C.c_double * 4), ('max_accel', C.c_double), ('max_speed', C.c_double),
                ('path_cum', C.c_void_p), ('path_cum_err', C.c_double), ('path_first_within', C.c_void_p),
                ('plan_cnt', C.c_void_p), ('plan_disc', C.c_void_p), ('plan_box', C.c_void_p), ('path_disc', C.c_void_p),
                ('plan_cap', C.c_int32), ('plan_steps', C.c_int32), ('plan_dl', C.c_double), ('plan_radius', C.c_double)]


class ClosedLoopC(C.Structure):
    """mirror of mpcx_closed_loop (include/mpcx.h); every pointer is a device address"""
    _PTRS = ['state', 'applied', 'obs6', 'path_xyyaw', 'path_cs', 'path_v', 'path_off', 'path_len', 'obs_off', 'obs_cnt',
             'obs_skip', 'traj_idx', 'target_ind', 'hit_idx', 'cut_len', 'hit_xy', 'xref', 'xbar', 'reaches_end',
             'x_sol', 'u_sol', 'status', 'iters', 'kkt']
    _fields_ = ([('P', C.c_int32), ('exchange', C.c_int32), ('dl', C.c_double)] + [(n, C.c_void_p) for n in _PTRS] +
                [('n_inst', C.c_int32), ('agents_local', C.c_int32), ('obs_local', C.c_void_p)] +
                # scripted traffic (n_actors = 0: none)
                [('n_actors', C.c_int32), ('pool_rows', C.c_int32), ('actors', C.c_void_p), ('actor_state', C.c_void_p), ('tape', C.c_void_p),
                 ('actor_row', C.c_void_p), ('ego_row', C.c_void_p), ('tape_rows', C.c_int64)])


class RunLogC(C.Structure):
    """mirror of mpcx_run_log (include/mpcx.h); every pointer is a device address"""
    _fields_ = ([('capacity', C.c_int32), ('reserved', C.c_int32), ('goal_dis', C.c_double), ('stop_speed', C.c_double)] +
                [(n, C.c_void_p) for n in ('rows_f64', 'rows_i32', 'steps', 'goal_step', 'contact_step', 'flags', 'min_clearance')])


class ClosedLoopOptsC(C.Structure):
    """mirror of mpcx_closed_loop_opts (include/mpcx.h); prev_len is a device address"""
    _fields_ = [('stop_mode', C.c_int32), ('reserved', C.c_int32), ('v_ref', C.c_double), ('prev_len', C.c_void_p)]


class RetireC(C.Structure):
    """mirror of mpcx_retire (include/mpcx.h): retirement at the goal; done and steps_driven are device addresses"""
    _fields_ = [('done', C.c_void_p), ('steps_driven', C.c_void_p), ('goal_dis', C.c_double), ('stop_speed', C.c_double)]


class SceneC(C.Structure):
    """mirror of mpcx_scene (include/mpcx.h): departure; absent is a device address (n_rows int32, one per pool row)"""
    _fields_ = [('absent', C.c_void_p), ('n_rows', C.c_int32), ('reserved', C.c_int32)]


class AdmitC(C.Structure):
    """mirror of mpcx_admit (include/mpcx.h): admission; wait, entered_step (P int32 each) and clock (1 int32) are device addresses"""
    _fields_ = [('wait', C.c_void_p), ('entered_step', C.c_void_p), ('clock', C.c_void_p), ('reserved', C.c_int32), ('gap', C.c_double)]


class RespawnC(C.Structure):
    """mirror of mpcx_respawn (include/mpcx.h): respawn; start_state (P,4 float64), start_idx (P), due (P,G), served (P), ep_i32 (P,G,8) and
    ep_f64 (P,G,2 float64) are device addresses"""
    _fields_ = [('generations', C.c_int32), ('reserved', C.c_int32), ('start_state', C.c_void_p), ('start_idx', C.c_void_p), ('due', C.c_void_p),
                ('served', C.c_void_p), ('ep_i32', C.c_void_p), ('ep_f64', C.c_void_p)]


class RoutesC(C.Structure):
    """mirror of mpcx_routes (include/mpcx.h): a route per vehicle; route_off, route_len (R), route_of (P,G), start_state (P,G,4 float64),
    start_idx (P,G) and the descriptor's own path_off, path_len (P) are device addresses"""
    _fields_ = [('n_routes', C.c_int32), ('reserved', C.c_int32), ('route_off', C.c_void_p), ('route_len', C.c_void_p), ('route_of', C.c_void_p),
                ('start_state', C.c_void_p), ('start_idx', C.c_void_p), ('path_off', C.c_void_p), ('path_len', C.c_void_p)]


class PrecedenceC(C.Structure):
    """mirror of mpcx_precedence (include/mpcx.h): right of way; prec (n_rows int32, a smaller word goes first) and stand (n_rows x 4
    float64, scratch) are device addresses"""
    _fields_ = [('prec', C.c_void_p), ('stand', C.c_void_p), ('n_rows', C.c_int32), ('mode', C.c_int32)]


PRECEDENCE_FIXED, PRECEDENCE_ENTRY = 1, 2       # mpcx_precedence.mode
PRECEDENCE_WINDOW = 64                          # MPCX_PRECEDENCE_WINDOW: the entry-order word is entered_step * 64 + window offset
PRECEDENCE_MAX_STEP = (2 ** 31 - 1 - (PRECEDENCE_WINDOW - 1)) // PRECEDENCE_WINDOW      # the largest entered_step whose word fits


class SignalsC(C.Structure):
    """mirror of mpcx_signals (include/mpcx.h): traffic signals; every pointer is a device address -- path_stop / path_group (n_points int32),
    plan_cycle / plan_amber (n_plans int32), plan_green (n_plans x n_groups x 2 int32), plan_of / tick / held (P int32)"""
    _fields_ = [('path_stop', C.c_void_p), ('path_group', C.c_void_p), ('plan_cycle', C.c_void_p), ('plan_amber', C.c_void_p),
                ('plan_green', C.c_void_p), ('plan_of', C.c_void_p), ('tick', C.c_void_p), ('held', C.c_void_p), ('brake', C.c_double),
                ('n_points', C.c_int32), ('n_plans', C.c_int32), ('n_groups', C.c_int32), ('reserved', C.c_int32)]


class ActuationC(C.Structure):
    """mirror of mpcx_actuation (include/mpcx.h): vehicle-actuated signals; every pointer is a device address -- phase_groups (n_ctrl x
    n_phases int32), phase_time (n_ctrl x n_phases x 3 int32), ctrl_time (n_ctrl x 3 int32), ctrl_of / lights / calls (n_junctions int32),
    jstate (n_junctions x 4 int32)"""
    _fields_ = [('phase_groups', C.c_void_p), ('phase_time', C.c_void_p), ('ctrl_time', C.c_void_p), ('ctrl_of', C.c_void_p),
                ('jstate', C.c_void_p), ('lights', C.c_void_p), ('calls', C.c_void_p), ('n_per', C.c_int32), ('n_junctions', C.c_int32),
                ('n_phases', C.c_int32), ('n_ctrl', C.c_int32), ('reserved', C.c_int32)]


class AdviceC(C.Structure):
    """mirror of mpcx_advice (include/mpcx.h): signal-aware approach speed; advised (n_rows = P float64, out) is a device address"""
    _fields_ = [('advised', C.c_void_p), ('v_cruise', C.c_double), ('v_min', C.c_double), ('reach', C.c_double), ('lead', C.c_int32),
                ('n_rows', C.c_int32)]


class IntentC(C.Structure):
    """mirror of mpcx_intent (include/mpcx.h): shared plans; share (n_rows = P int32, nonzero = the agent shares its plan) and frames
    (n_rows int32, out) are device addresses"""
    _fields_ = [('share', C.c_void_p), ('frames', C.c_void_p), ('n_rows', C.c_int32), ('reserved', C.c_int32)]


class ReservationC(C.Structure):
    """mirror of mpcx_reservation (include/mpcx.h): crossing reservations; every pointer is a device address -- path_exit (n_points int32),
    conflict / lane (n_groups int32), mgr_time (n_mgr x 2 int32), mgr_of / clock / occupied / queued (n_junctions int32), grant / since
    (P int32)"""
    _fields_ = [('path_exit', C.c_void_p), ('conflict', C.c_void_p), ('lane', C.c_void_p), ('mgr_time', C.c_void_p), ('mgr_of', C.c_void_p),
                ('grant', C.c_void_p), ('since', C.c_void_p), ('clock', C.c_void_p), ('occupied', C.c_void_p), ('queued', C.c_void_p),
                ('n_per', C.c_int32), ('n_junctions', C.c_int32), ('n_mgr', C.c_int32), ('reserved', C.c_int32)]


class FollowingC(C.Structure):
    """mirror of mpcx_following (include/mpcx.h): car following; leader (n_rows = P int32, out), gap and cap (n_rows float64, out) are
    device addresses.  Not a row of STAGES: the stage attaches to the context (Context.set_following), not to an entry point"""
    _fields_ = [('leader', C.c_void_p), ('gap', C.c_void_p), ('cap', C.c_void_p), ('standstill', C.c_double), ('time_gap', C.c_double),
                ('brake', C.c_double), ('v_min', C.c_double), ('lateral', C.c_double), ('heading', C.c_double), ('reach', C.c_int32),
                ('n_rows', C.c_int32), ('reserved', C.c_int32)]


class SafetyC(C.Structure):
    """mirror of mpcx_safety (include/mpcx.h): the near-miss log; every pointer is a device address -- partner, ttc_row, ttc_frame, tick,
    enc_row, n_events (n_rows = P int32), clearance (n_rows float64), ev_i32 (n_rows x capacity x 8 int32), ev_f64 (n_rows x capacity x 2
    float64), row_agent (n_pool int32, in).  Not a row of STAGES: the stage attaches to the context (Context.set_safety)"""
    _fields_ = [('partner', C.c_void_p), ('clearance', C.c_void_p), ('ttc_row', C.c_void_p), ('ttc_frame', C.c_void_p), ('tick', C.c_void_p),
                ('enc_row', C.c_void_p), ('n_events', C.c_void_p), ('ev_i32', C.c_void_p), ('ev_f64', C.c_void_p), ('row_agent', C.c_void_p),
                ('near', C.c_double), ('ttc_frames', C.c_int32), ('capacity', C.c_int32), ('n_rows', C.c_int32), ('n_pool', C.c_int32),
                ('reserved', C.c_int32)]


class SightC(C.Structure):
    """mirror of mpcx_sight (include/mpcx.h): line of sight; every pointer is a device address -- sight (n_rows = P uint64, out), n_seen,
    n_hidden (n_rows int32, out), hp (rows x 3 float64), hp_off (n_occ + 1 int32), box (n_occ x 4 float64), set_off (n_sets + 1 int32),
    set_of (n_rows int32), heard (n_pool int32 or None).  Not a row of STAGES: the stage attaches to the context (Context.set_sight)"""
    _fields_ = [('sight', C.c_void_p), ('n_seen', C.c_void_p), ('n_hidden', C.c_void_p), ('hp', C.c_void_p), ('hp_off', C.c_void_p),
                ('box', C.c_void_p), ('set_off', C.c_void_p), ('set_of', C.c_void_p), ('heard', C.c_void_p), ('range', C.c_double),
                ('n_occ', C.c_int32), ('n_sets', C.c_int32), ('n_rows', C.c_int32), ('n_pool', C.c_int32), ('reserved', C.c_int32)]


class KeepClearC(C.Structure):
    """mirror of mpcx_keepclear (include/mpcx.h): keep clear; every pointer is a device address -- path_move / path_exit (n_points int32),
    conflict (n_moves int32), boxed / waited (P int32), occupied / n_boxed (n_junctions int32).  Not a row of STAGES: the stage attaches to
    the context (Context.set_keepclear)"""
    _fields_ = [('path_move', C.c_void_p), ('path_exit', C.c_void_p), ('conflict', C.c_void_p), ('boxed', C.c_void_p), ('waited', C.c_void_p),
                ('occupied', C.c_void_p), ('n_boxed', C.c_void_p), ('detect', C.c_int32), ('n_per', C.c_int32), ('n_junctions', C.c_int32),
                ('n_moves', C.c_int32), ('n_points', C.c_int32), ('reserved', C.c_int32)]


class PriorityC(C.Structure):
    """mirror of mpcx_priority (include/mpcx.h): priority road; every pointer is a device address -- path_stop / path_move / path_exit
    (n_points int32), conflict / rank (n_moves int32), gap (n_moves float64), waited / yielding / blocker (P int32), lag (P float64),
    occupied / n_yielding (n_junctions int32).  Not a row of STAGES: the stage attaches to the context (Context.set_priority)"""
    _fields_ = [('path_stop', C.c_void_p), ('path_move', C.c_void_p), ('path_exit', C.c_void_p), ('conflict', C.c_void_p), ('rank', C.c_void_p),
                ('gap', C.c_void_p), ('waited', C.c_void_p), ('yielding', C.c_void_p), ('blocker', C.c_void_p), ('lag', C.c_void_p),
                ('occupied', C.c_void_p), ('n_yielding', C.c_void_p), ('v_floor', C.c_double), ('brake', C.c_double), ('detect', C.c_int32),
                ('n_per', C.c_int32), ('n_junctions', C.c_int32), ('n_moves', C.c_int32), ('n_points', C.c_int32), ('reserved', C.c_int32)]


class StopSignC(C.Structure):
    """mirror of mpcx_stopsign (include/mpcx.h): stop signs; every pointer is a device address -- path_stop / path_move / path_exit
    (n_points int32), conflict / lane / sign (n_moves int32), gap (n_moves float64), stopped_at / go / stopping / blocker (P int32), lag
    (P float64), clock / ran / occupied / n_waiting (n_junctions int32).  Not a row of STAGES: the stage attaches to the context
    (Context.set_stopsign)"""
    _fields_ = [('path_stop', C.c_void_p), ('path_move', C.c_void_p), ('path_exit', C.c_void_p), ('conflict', C.c_void_p), ('lane', C.c_void_p),
                ('sign', C.c_void_p), ('gap', C.c_void_p), ('stopped_at', C.c_void_p), ('go', C.c_void_p), ('stopping', C.c_void_p),
                ('clock', C.c_void_p), ('ran', C.c_void_p), ('lag', C.c_void_p), ('blocker', C.c_void_p), ('occupied', C.c_void_p),
                ('n_waiting', C.c_void_p), ('v_stop', C.c_double), ('brake', C.c_double), ('v_floor', C.c_double), ('zone', C.c_int32),
                ('detect', C.c_int32), ('patience', C.c_int32), ('n_per', C.c_int32), ('n_junctions', C.c_int32), ('n_moves', C.c_int32),
                ('n_points', C.c_int32), ('reserved', C.c_int32)]


class BrakingC(C.Structure):
    """mirror of mpcx_braking (include/mpcx.h): firm hold; firm / overran (P int32) and brake_cap (P float64) are device addresses.  Not a
    row of STAGES: the stage attaches to the context (Context.set_braking)"""
    _fields_ = [('brake', C.c_double), ('setback', C.c_double), ('firm', C.c_void_p), ('overran', C.c_void_p), ('brake_cap', C.c_void_p)]


PRIORITY_PER_MAX = 64                           # MPCX_PRIORITY_PER_MAX: agents per junction under the priority rule
STOPSIGN_PER_MAX = 64                           # MPCX_STOPSIGN_PER_MAX: agents per junction under stop signs
KEEPCLEAR_PER_MAX = 64                          # MPCX_KEEPCLEAR_PER_MAX: agents per junction under keep clear
SIGHT_WINDOW = 64                               # window offsets a word of mpcx_sight.sight holds
# the words of an event record of the near-miss log (ev_i32[q][e][0..7]; ev_f64[q][e] = the minimum clearance, the agent's speed at opening)
SAFETY_I32 = ('open', 'last', 'row', 'row_agent', 'path_off', 'partner_path_off', 'traj_idx', 'ttc_frame')
SAFETY_F64 = ('min_clearance', 'v')
# the columns of mpcx_safety_summary's tables (out_i64[b][i][j][0..2], out_f64[b][i][j][0..1])
SAFETY_SUMMARY_I64 = ('events', 'contacts', 'predicted')
SAFETY_SUMMARY_F64 = ('min_clearance', 'min_ttc')
MAX_REMAINING = 1024                            # MPCX_MAX_REMAINING: the largest mpcx_following.reach
SIGNAL_GROUPS_MAX = 16                          # MPCX_SIGNAL_GROUPS_MAX
RESERVE_PER_MAX = 64                            # MPCX_RESERVE_PER_MAX: agents per junction under reservations
ACTUATION_PHASES_MAX = 8                        # MPCX_ACTUATION_PHASES_MAX
STAGE_GREEN, STAGE_AMBER, STAGE_ALL_RED = 0, 1, 2       # mpcx_actuation.jstate[j][1]
LIGHT_GREEN, LIGHT_AMBER, LIGHT_RED = 0, 1, 2   # MPCX_SIGNAL_*: two bits per group in mpcx_actuation.lights
HELD_FREE, HELD_RED, HELD_AMBER = 0, 1, 2       # mpcx_signals.held


# the words of an episode record (ep_i32[q][g][0..6]; word 7 is 0, with routes the episode's route: EPISODE_ROUTE_WORD; ep_f64[q][g][0], one
# reserved)
EPISODE_I32 = ('entered', 'arrived', 'steps_driven', 'row_end', 'contact_step', 'flags', 'due')
EPISODE_F64 = ('min_clearance',)
EPISODE_ROUTE_WORD = 7
# the columns of mpcx_episode_summary's integer table (out_i64[b][r][0..3]); out_f64[b][r] is the minimum of min_clearance
SUMMARY_I64 = ('count', 'contacts', 'delay_sum', 'steps_driven_sum')


STOP_CUT, STOP_SPEED = 0, 1     # mpcx_closed_loop_opts.stop_mode
STOP_MODES = {'cut': STOP_CUT, 'speed': STOP_SPEED}
NO_STOP = 999                   # MPCX_NO_STOP: the stop index lib/mpc_with_speed.py:281 reads as "no stop"


# the columns of a run-log row (rows_f64[s][q][0..7], rows_i32[s][q][0..5]; two reserved integer columns follow)
RUN_LOG_F64 = ('x', 'y', 'v', 'yaw', 'accel', 'steer', 'xref_deviation', 'clearance')
RUN_LOG_I32 = ('traj_idx', 'target_ind', 'cut_len', 'hit_idx', 'status', 'iters')
RUN_LOG_ROW_BYTES = 96          # per agent and step
RUN_LOG_AGENT_BYTES = 24        # per agent: steps, goal_step, contact_step, flags, min_clearance


class TrafficActorC(C.Structure):
    """mirror of mpcx_traffic_actor (include/mpcx.h): the constants of one scripted vehicle"""
    _fields_ = ([(n, C.c_int32) for n in ('kind', 'direction', 'turning', 'tape_rows', 'tape_off', 'tape_stride')] +
                [(n, C.c_double) for n in ('speed', 'offset', 'counter_dt', 'model_dt', 'L', 'x_turn', 'arc')])


class AstarSearchC(C.Structure):
    """mirror of mpcx_astar_search (include/mpcx.h)"""
    _fields_ = [('start', C.c_double * 3), ('goal_box', C.c_double * 4), ('goal_point', C.c_double * 3), ('allowed_dtheta', C.c_double),
                ('wh', C.c_double * 5), ('wc', C.c_double * 4), ('hp_norm', C.c_void_p),
                ('variant', C.c_int32), ('max_expansions', C.c_int32), ('ov_off', C.c_int32), ('ov_cnt', C.c_int32)]


class AstarBuffersC(C.Structure):
    """mirror of mpcx_astar_buffers (include/mpcx.h); every pointer is a device address"""
    _fields_ = ([(n, C.c_int32) for n in ('heap_cap', 'table_cap', 'log_cap', 'push_cap', 'path_cap')] +
                [(n, C.c_void_p) for n in ('heap', 'table', 'log', 'push_log', 'path', 'cost', 'miss', 'status', 'n_exp', 'n_push', 'path_len', 'path_prim')])


# the same struct as a numpy record (plan_many_device fills thousands of rows without a Python loop per field)
import numpy as _np
ASTAR_SEARCH_DTYPE = _np.dtype([('start', '<f8', 3), ('goal_box', '<f8', 4), ('goal_point', '<f8', 3), ('allowed_dtheta', '<f8'),
                                ('wh', '<f8', 5), ('wc', '<f8', 4), ('hp_norm', '<u8'), ('variant', '<i4'), ('max_expansions', '<i4'),
                                ('ov_off', '<i4'), ('ov_cnt', '<i4')])
assert ASTAR_SEARCH_DTYPE.itemsize == C.sizeof(AstarSearchC)
# mpcx_traffic_actor as a numpy record (actor tables of thousands of rows are filled column by column)
TRAFFIC_ACTOR_DTYPE = _np.dtype([(n, '<i4') for n in ('kind', 'direction', 'turning', 'tape_rows', 'tape_off', 'tape_stride')] +
                                [(n, '<f8') for n in ('speed', 'offset', 'counter_dt', 'model_dt', 'L', 'x_turn', 'arc')])
assert TRAFFIC_ACTOR_DTYPE.itemsize == C.sizeof(TrafficActorC)
TRAFFIC_TINTERSECTION, TRAFFIC_ROUNDABOUT, TRAFFIC_ARTERIAL, TRAFFIC_TAPE = 0, 1, 2, 3
MAX_OBS = 16        # MPCX_MAX_OBS: moving obstacles seen by one ego
ASTAR_BASE, ASTAR_MODIFIED, ASTAR_MULTI_LANE, ASTAR_ROUNDABOUT, ASTAR_SINGLE_LANE = 0, 1, 2, 3, 4
ASTAR_VARIANTS = {'base': ASTAR_BASE, 'modified': ASTAR_MODIFIED, 'multi_lane': ASTAR_MULTI_LANE, 'roundabout': ASTAR_ROUNDABOUT,
                  'single_lane': ASTAR_SINGLE_LANE}
ASTAR_FOUND, ASTAR_EXHAUSTED, ASTAR_CAPACITY, ASTAR_MISS, ASTAR_PATH_CAPACITY = 0, 1, 2, 3, 4
COMM_ID_BYTES = 128
SHARD_INSTANCES, SHARD_AGENTS = 1, 2


class Stage(NamedTuple):
    """one optional stage of the device closed loop, as the Python layer knows it"""
    key: str                    # the keyword of Context.closed_loop_run, and IntersectionBatch's attribute `_<key>` (log: `log.c`)
    struct: type                # the ctypes mirror of ...
    c_name: str                 # ... this struct of include/mpcx.h
    suffix: str                 # mpcx_closed_loop_run_<suffix>: the entry point that introduced it
    doc: str                    # its paragraph of Context.closed_loop_run's docstring
    dependents: tuple = ()      # the stages that live on it: switched off with it (direct ones; stage_dependents() takes the closure)
    entry_dependents: tuple = ()    # ... and those that do so only while right of way is by order of entry (PRECEDENCE_ENTRY)


# THE list of the loop's stages on the Python side, in the order of LoopArgs (csrc/mpcx_loop.hip) and of the entry points' parameters: the
# prototypes of load(), the keywords of Context.closed_loop_run and what IntersectionBatch passes and tears down are all read from it
STAGES = (
    Stage('log', RunLogC, 'mpcx_run_log', 'logged',
          'a _lib.RunLogC -- every step then ends with the run log\'s record stage (mpcx_closed_loop_run_logged).'),
    Stage('opts', ClosedLoopOptsC, 'mpcx_closed_loop_opts', 'opts',
          'a _lib.ClosedLoopOptsC -- the stop mode (mpcx_closed_loop_run_opts); None = the path cut.'),
    Stage('retire', RetireC, 'mpcx_retire', 'retire',
          'a _lib.RetireC -- agents are retired at their goal (mpcx_closed_loop_run_retire); None = they are driven on.', ('scene',)),
    Stage('scene', SceneC, 'mpcx_scene', 'scene',
          'a _lib.SceneC -- departure: pool rows with absent != 0 are out of the scene and an arrival sets the agent\'s own word '
          '(mpcx_closed_loop_run_scene; refused without retire); None = arrived cars stay in the scene.', ('admit', 'precedence')),
    Stage('admit', AdmitC, 'mpcx_admit', 'admit',
          'a _lib.AdmitC -- admission: waiting agents enter on their schedule once their start pose is clear (mpcx_closed_loop_run_admit; '
          'refused without scene); None = everybody is in from the start.', ('respawn',), ('precedence',)),
    Stage('respawn', RespawnC, 'mpcx_respawn', 'respawn',
          'a _lib.RespawnC -- respawn: an arrived agent\'s slot is reset for the next vehicle of its stream and handed back to the '
          'admission gate (mpcx_closed_loop_run_respawn; refused without admit); None = a departed slot stays empty.', ('routes',)),
    Stage('routes', RoutesC, 'mpcx_routes', 'routes',
          'a _lib.RoutesC -- every vehicle of a slot takes its own route from its own start pose (mpcx_closed_loop_run_routes; refused '
          'without respawn); None = a slot keeps its route.'),
    Stage('precedence', PrecedenceC, 'mpcx_precedence', 'precedence',
          'a _lib.PrecedenceC -- right of way: an agent sees the present rows whose word is larger than its own as standing cars '
          '(mpcx_closed_loop_run_precedence; refused without scene, and in ENTRY mode without admit); None = everybody yields to everybody.'),
    Stage('signals', SignalsC, 'mpcx_signals', 'signals',
          'a _lib.SignalsC -- traffic signals: one more launch behind the conflict search holds agents at their stop lines '
          '(mpcx_closed_loop_run_signals; needs none of the others); None = no signals.', ('actuation', 'reservation', 'advice')),
    Stage('actuation', ActuationC, 'mpcx_actuation', 'actuated',
          'a _lib.ActuationC -- vehicle-actuated signals: a controller per junction takes the place of the signals\' fixed plan '
          '(mpcx_closed_loop_run_actuated; refused without signals); None = the signals\' own plan.'),
    Stage('advice', AdviceC, 'mpcx_advice', 'advised',
          'a _lib.AdviceC -- signal-aware approach speed: one more launch between the window stage and the QP caps the speed reference '
          'of an agent that would reach its stop line on red (mpcx_closed_loop_run_advised; refused without signals under a fixed plan, with '
          'actuation and outside speed mode); None = no advice.'),
    Stage('intent', IntentC, 'mpcx_intent', 'intent',
          'a _lib.IntentC -- shared plans: one more launch between the prediction and the conflict search predicts a sharing agent from '
          'its last MPC solution instead of its last controls (mpcx_closed_loop_run_intent; refused in the agent-sharded layout); None = every '
          'agent is predicted from its last controls.'),
    Stage('reservation', ReservationC, 'mpcx_reservation', 'reserved',
          'a _lib.ReservationC -- crossing reservations: a manager per junction takes the place of the signals\' fixed plan and '
          'admits only compatible movements (mpcx_closed_loop_run_reserved; refused without signals, with a plan, actuation or advice); None = '
          'no reservations.'),
)
STAGE_KEYS = tuple(st.key for st in STAGES)
# rung k of the ladder takes the first k stages' structs; Context.closed_loop_run calls the last with NULL for what is off
LOOP_ENTRY_POINTS = ['mpcx_closed_loop_run'] + ['mpcx_closed_loop_run_' + st.suffix for st in STAGES]


def stage_dependents(key: str, entry_order: bool = False) -> set:
    """every stage that is switched off with stage `key` (itself not included); entry_order: right of way is on in PRECEDENCE_ENTRY mode"""
    st = STAGES[STAGE_KEYS.index(key)]
    out = set()
    for k in st.dependents + (st.entry_dependents if entry_order else ()):
        out |= {k} | stage_dependents(k, entry_order)
    return out


def stage_structs(stages: dict) -> list:
    """the keyword arguments of Context.closed_loop_run as the widest entry point takes them: one struct or None per stage, in order"""
    unknown = sorted(set(stages) - set(STAGE_KEYS))
    if unknown:
        raise TypeError('closed_loop_run() got an unexpected keyword argument %s: the stages are %s'
                        % (', '.join(map(repr, unknown)), ', '.join(STAGE_KEYS)))
    return [stages.get(k) for k in STAGE_KEYS]


EXPORTS = ['mpcx_create', 'mpcx_destroy', 'mpcx_last_error', 'mpcx_version', 'mpcx_set_mpc_params', 'mpcx_qp_solve_batch',
           'mpcx_mpc_prepare_batch', 'mpcx_search_model_create', 'mpcx_search_model_destroy', 'mpcx_expand_batch',
           'mpcx_interaction_batch', 'mpcx_moving_collision_batch', 'mpcx_plant_step_batch', 'mpcx_transform_batch',
           'mpcx_cutoff_index_batch', 'mpcx_predict_obstacles_batch', 'mpcx_selftest_wave_ops', 'mpcx_selftest_mfma', 'mpcx_profile_qp',
           'mpcx_profile_qp_read', 'mpcx_set_instance_tuning', 'mpcx_set_qp_solver', 'mpcx_qp_set_order_hint', 'mpcx_expand_multi_batch',
           'mpcx_comm_unique_id', 'mpcx_comm_init', 'mpcx_comm_destroy', 'mpcx_allgather_states', 'mpcx_closed_loop_stats',
           'mpcx_mpc_prepare_batch_ov', 'mpcx_set_linearisation_passes', 'mpcx_set_step_fusion', 'mpcx_qp_set_plain_rounds', 'mpcx_astar_batch',
           'mpcx_traffic_step_batch', 'mpcx_record_step_batch', 'mpcx_mpc_prepare_batch_stop', 'mpcx_record_step_batch_goal',
           'mpcx_admit_step_batch', 'mpcx_respawn_step_batch', 'mpcx_respawn_step_batch_routes', 'mpcx_episode_summary',
           'mpcx_admit_step_batch_precedence', 'mpcx_signal_step_batch', 'mpcx_closed_loop_queue', 'mpcx_interaction_prediction',
           'mpcx_actuated_step_batch', 'mpcx_advise_step_batch', 'mpcx_interaction_batch_intent',
           'mpcx_reserve_step_batch', 'mpcx_set_following', 'mpcx_follow_step_batch', 'mpcx_follow_cap_step_batch',
           'mpcx_set_safety', 'mpcx_safety_step_batch', 'mpcx_safety_summary', 'mpcx_set_sight', 'mpcx_sight_step_batch',
           'mpcx_set_keepclear', 'mpcx_keepclear_step_batch', 'mpcx_set_priority', 'mpcx_priority_step_batch', 'mpcx_set_stopsign', 'mpcx_stopsign_step_batch',
           'mpcx_set_braking', 'mpcx_brake_mark_step_batch', 'mpcx_brake_clamp_step_batch'] + LOOP_ENTRY_POINTS


def load():
    """Load libmpcx.so and declare the prototypes of include/mpcx.h. Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('libmpcx.so not built (%s): run `python -c "import __graft_entry__ as g; g.build()"` '
                           'or `make -C mpc_for_av_at_intersection_amd/csrc`; there is no CPU fallback' % LIB_PATH)
    # torch first: libmpcx.so must bind to the HIP runtime torch ships (same SONAME), not open a second copy
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    lib.mpcx_create.restype = vp; lib.mpcx_create.argtypes = [i32, vp]
    lib.mpcx_destroy.restype = None; lib.mpcx_destroy.argtypes = [vp]
    lib.mpcx_last_error.restype = C.c_char_p; lib.mpcx_last_error.argtypes = [vp]
    lib.mpcx_version.restype = C.c_char_p; lib.mpcx_version.argtypes = []
    lib.mpcx_set_mpc_params.restype = i32; lib.mpcx_set_mpc_params.argtypes = [vp, C.POINTER(MpcParamsC)]
    lib.mpcx_qp_solve_batch.restype = i32; lib.mpcx_qp_solve_batch.argtypes = [vp, i32] + [vp] * 10
    lib.mpcx_mpc_prepare_batch.restype = i32
    lib.mpcx_mpc_prepare_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp]
    lib.mpcx_mpc_prepare_batch_ov.restype = i32
    lib.mpcx_mpc_prepare_batch_ov.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, C.c_int64, vp, vp, vp]
    lib.mpcx_set_linearisation_passes.restype = i32; lib.mpcx_set_linearisation_passes.argtypes = [vp, i32]
    lib.mpcx_set_step_fusion.restype = i32; lib.mpcx_set_step_fusion.argtypes = [vp, i32]
    lib.mpcx_qp_set_plain_rounds.restype = i32; lib.mpcx_qp_set_plain_rounds.argtypes = [vp, i32]
    lib.mpcx_astar_batch.restype = i32
    lib.mpcx_astar_batch.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    lib.mpcx_search_model_create.restype = vp
    lib.mpcx_search_model_create.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.mpcx_search_model_destroy.restype = None; lib.mpcx_search_model_destroy.argtypes = [vp]
    lib.mpcx_expand_batch.restype = i32; lib.mpcx_expand_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.mpcx_interaction_batch.restype = i32
    lib.mpcx_interaction_batch.argtypes = [vp, C.POINTER(InteractionParamsC), i32] + [vp] * 6 + [i32] + [vp] * 8
    lib.mpcx_moving_collision_batch.restype = i32
    lib.mpcx_moving_collision_batch.argtypes = [vp, C.POINTER(InteractionParamsC), i32] + [vp] * 8 + [i32] + [vp] * 6
    lib.mpcx_plant_step_batch.restype = i32; lib.mpcx_plant_step_batch.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.mpcx_transform_batch.restype = i32; lib.mpcx_transform_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.mpcx_cutoff_index_batch.restype = i32
    lib.mpcx_cutoff_index_batch.argtypes = [vp, i32, vp, vp, vp, vp, C.c_double, vp]
    lib.mpcx_predict_obstacles_batch.restype = i32
    lib.mpcx_predict_obstacles_batch.argtypes = [vp, i32, i32, C.c_double, C.c_double, vp, vp]
    lib.mpcx_selftest_wave_ops.restype = i32; lib.mpcx_selftest_wave_ops.argtypes = [vp, vp, vp]
    lib.mpcx_selftest_mfma.restype = i32; lib.mpcx_selftest_mfma.argtypes = [vp, vp, vp, vp]
    for k, name in enumerate(LOOP_ENTRY_POINTS):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp, C.POINTER(InteractionParamsC), C.POINTER(ClosedLoopC)] + [C.POINTER(st.struct) for st in STAGES[:k]] + [i32, i32]
    lib.mpcx_profile_qp.restype = i32; lib.mpcx_profile_qp.argtypes = [vp, i32]
    lib.mpcx_profile_qp_read.restype = i32
    lib.mpcx_profile_qp_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.mpcx_set_instance_tuning.restype = i32; lib.mpcx_set_instance_tuning.argtypes = [vp, vp, i32]
    lib.mpcx_set_qp_solver.restype = i32; lib.mpcx_set_qp_solver.argtypes = [vp, i32]
    lib.mpcx_qp_set_order_hint.restype = i32; lib.mpcx_qp_set_order_hint.argtypes = [vp, vp, vp, vp]
    lib.mpcx_expand_multi_batch.restype = i32; lib.mpcx_expand_multi_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcx_comm_unique_id.restype = i32; lib.mpcx_comm_unique_id.argtypes = [vp]
    lib.mpcx_comm_init.restype = i32; lib.mpcx_comm_init.argtypes = [vp, i32, i32, vp]
    lib.mpcx_comm_destroy.restype = i32; lib.mpcx_comm_destroy.argtypes = [vp]
    lib.mpcx_allgather_states.restype = i32; lib.mpcx_allgather_states.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.mpcx_closed_loop_stats.restype = i32; lib.mpcx_closed_loop_stats.argtypes = [vp, C.POINTER(C.c_int64), i32]
    lib.mpcx_closed_loop_queue.restype = i32; lib.mpcx_closed_loop_queue.argtypes = [vp, i32, vp, vp]
    lib.mpcx_interaction_prediction.restype = i32; lib.mpcx_interaction_prediction.argtypes = [vp, i32, i32, vp]
    lib.mpcx_traffic_step_batch.restype = i32; lib.mpcx_traffic_step_batch.argtypes = [vp, i32, vp, vp, vp, C.c_int64, vp, i32, vp]
    lib.mpcx_record_step_batch.restype = i32
    lib.mpcx_record_step_batch.argtypes = [vp, C.POINTER(InteractionParamsC), i32] + [vp] * 12 + [i32] + [vp] * 4 + [C.POINTER(RunLogC)]
    lib.mpcx_mpc_prepare_batch_stop.restype = i32
    lib.mpcx_mpc_prepare_batch_stop.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, C.c_int64, vp, C.c_double, vp, vp, vp, vp]
    lib.mpcx_record_step_batch_goal.restype = i32
    lib.mpcx_record_step_batch_goal.argtypes = [vp, C.POINTER(InteractionParamsC), i32] + [vp] * 12 + [i32] + [vp] * 5 + [C.POINTER(RunLogC)]
    lib.mpcx_admit_step_batch.restype = i32
    lib.mpcx_admit_step_batch.argtypes = [vp, C.POINTER(InteractionParamsC), i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, C.c_int64, vp,
                                          C.POINTER(AdmitC)]
    lib.mpcx_respawn_step_batch.restype = i32
    lib.mpcx_respawn_step_batch.argtypes = [vp, i32] + [vp] * 9 + [i32, C.POINTER(RunLogC), C.POINTER(RetireC), C.POINTER(AdmitC),
                                                                   C.POINTER(RespawnC)]
    lib.mpcx_respawn_step_batch_routes.restype = i32
    lib.mpcx_respawn_step_batch_routes.argtypes = [vp, i32] + [vp] * 9 + [i32, C.POINTER(RunLogC), C.POINTER(RetireC), C.POINTER(AdmitC),
                                                                          C.POINTER(RespawnC), C.POINTER(RoutesC), i32]
    lib.mpcx_episode_summary.restype = i32
    lib.mpcx_episode_summary.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.mpcx_admit_step_batch_precedence.restype = i32
    lib.mpcx_admit_step_batch_precedence.argtypes = [vp, C.POINTER(InteractionParamsC), i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp,
                                                     C.c_int64, vp, C.POINTER(AdmitC), C.POINTER(PrecedenceC)]
    lib.mpcx_signal_step_batch.restype = i32
    lib.mpcx_signal_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(SignalsC)]
    lib.mpcx_actuated_step_batch.restype = i32
    lib.mpcx_actuated_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(SignalsC), C.POINTER(ActuationC)]
    lib.mpcx_advise_step_batch.restype = i32
    lib.mpcx_advise_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, C.POINTER(SignalsC), C.POINTER(AdviceC), vp]
    lib.mpcx_interaction_batch_intent.restype = i32
    lib.mpcx_interaction_batch_intent.argtypes = ([vp, C.POINTER(InteractionParamsC), i32] + [vp] * 6 + [i32] + [vp] * 8 + [vp] * 4 +
                                                  [C.POINTER(IntentC)])
    lib.mpcx_reserve_step_batch.restype = i32
    lib.mpcx_reserve_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(SignalsC), C.POINTER(ReservationC)]
    lib.mpcx_set_following.restype = i32; lib.mpcx_set_following.argtypes = [vp, C.POINTER(FollowingC)]
    lib.mpcx_follow_step_batch.restype = i32
    lib.mpcx_follow_step_batch.argtypes = [vp, i32, C.c_double, i32] + [vp] * 7 + [i32] + [vp] * 5 + [C.POINTER(FollowingC)]
    lib.mpcx_follow_cap_step_batch.restype = i32
    lib.mpcx_follow_cap_step_batch.argtypes = [vp, i32, vp, C.POINTER(FollowingC), vp]
    lib.mpcx_set_safety.restype = i32; lib.mpcx_set_safety.argtypes = [vp, C.POINTER(SafetyC)]
    lib.mpcx_safety_step_batch.restype = i32
    lib.mpcx_safety_step_batch.argtypes = [vp, C.POINTER(InteractionParamsC), i32] + [vp] * 4 + [i32] + [vp] * 6 + [C.POINTER(SafetyC)]
    lib.mpcx_safety_summary.restype = i32
    lib.mpcx_safety_summary.argtypes = [vp, i32, i32, i32, i32, vp, C.c_double] + [vp] * 5
    lib.mpcx_set_sight.restype = i32; lib.mpcx_set_sight.argtypes = [vp, C.POINTER(SightC)]
    lib.mpcx_sight_step_batch.restype = i32
    lib.mpcx_sight_step_batch.argtypes = [vp, i32, vp, vp, i32] + [vp] * 5 + [C.POINTER(SightC)]
    lib.mpcx_set_keepclear.restype = i32; lib.mpcx_set_keepclear.argtypes = [vp, C.POINTER(KeepClearC)]
    lib.mpcx_keepclear_step_batch.restype = i32
    lib.mpcx_keepclear_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(SignalsC), C.POINTER(KeepClearC)]
    lib.mpcx_set_priority.restype = i32; lib.mpcx_set_priority.argtypes = [vp, C.POINTER(PriorityC)]
    lib.mpcx_priority_step_batch.restype = i32
    lib.mpcx_priority_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(PriorityC)]
    lib.mpcx_set_stopsign.restype = i32; lib.mpcx_set_stopsign.argtypes = [vp, C.POINTER(StopSignC)]
    lib.mpcx_stopsign_step_batch.restype = i32
    lib.mpcx_stopsign_step_batch.argtypes = [vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(StopSignC)]
    lib.mpcx_set_braking.restype = i32; lib.mpcx_set_braking.argtypes = [vp, C.POINTER(BrakingC)]
    lib.mpcx_brake_mark_step_batch.restype = i32
    lib.mpcx_brake_mark_step_batch.argtypes = [vp, i32, C.c_double, i32] + [vp] * 7 + [i32] + [vp] * 3 + [C.POINTER(BrakingC)]
    lib.mpcx_brake_clamp_step_batch.restype = i32
    lib.mpcx_brake_clamp_step_batch.argtypes = [vp, i32, C.c_double] + [vp] * 8 + [i32, C.POINTER(BrakingC), vp]
    _lib = lib
    return lib
