"""GPU test of the switch-on and switch-off methods of IntersectionBatch over the stage table (_lib.STAGES): one script walks every row of
the table's dependents and every "replaces" rule of the switch-on methods, and after every call the set of stages that are on is the one
written beside it.  One instance of eight agents on the stock routes, T = 20, speed mode (the batch of tests/test_gpu_entry_points.py: the
smallest on which every stage can be switched on).  The table itself is tests/test_stage_table_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WAIT = np.array([-1, -1, 0, 2, -1, -1, 7, -1])
STAGES = ('opts', 'retire', 'scene', 'admit', 'respawn', 'routes', 'precedence', 'signals', 'actuation', 'advice', 'intent', 'reservation')
OPEN = ('opts', 'retire', 'scene', 'admit', 'respawn', 'routes', 'precedence')
BASE_KEYS = {'state', 'applied', 'traj_idx', 'target_ind', 'prev_cut', 'x', 'u', 'status', 'iters', 'kkt', 'hit_idx', 'hit_xy', 'cut_len',
             'xref', 'reaches_end', 'xbar'}


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def _on(sim, *want):
    """the stages that are on are exactly `want` (speed mode: the stop-mode struct always is)"""
    have = tuple(k for k in STAGES if getattr(sim, '_' + k) is not None)
    assert have == want and sim._desc is None, (have, want)


def _open(sim, order):
    """retirement, scene, admission, respawn with a route per vehicle (the slot's own, twice) and right of way: the open intersection"""
    sim.retire_at_goal(leave_scene=True)
    sim.respawn_on_schedule(np.zeros((1, 8, 2), dtype=np.int64), gap=0.0, route=np.tile(np.arange(8)[None, :, None], (1, 1, 2)))
    sim.give_way(order)


def _run(sim):
    sim.run(2)
    sim.check()
    assert sim._desc is not None        # (cached: every switch below has to drop it again, which _on() looks at)


def test_switches_walk_the_table(ctx):
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch, two_phase_controller, two_phase_plan
    routes, dl, cd = stock_routes(ctx)
    sim = synthetic_batch(ctx, B=1, A=8, T=20, seed=11, routes=routes, dl=dl, cd=cd, stop_mode='speed')
    fixed = np.arange(8)
    plan, ctrl, mgr = two_phase_plan(cycle=100, green=30, amber=8), two_phase_controller(10, 40, 5, 8, 12, detect=144), dict(detect=144, patience=0)
    _on(sim, 'opts')
    # ---- the stages that live on retirement: switched on one by one
    sim.retire_at_goal(); _on(sim, 'opts', 'retire')
    sim.retire_at_goal(leave_scene=True); _on(sim, 'opts', 'retire', 'scene')
    sim.respawn_on_schedule(np.zeros((1, 8, 2), dtype=np.int64)); _on(sim, 'opts', 'retire', 'scene', 'admit', 'respawn')
    _open(sim, 'entry'); _on(sim, *OPEN)
    assert sim._precedence.mode == _lib.PRECEDENCE_ENTRY
    _run(sim)                                                   # (1) all of retire / scene / admit / respawn / routes / precedence on
    sim.stop_respawning(); _on(sim, 'opts', 'retire', 'scene', 'admit', 'precedence')          # respawn -> routes
    sim.enter_now(); _on(sim, 'opts', 'retire', 'scene')       # admit, by order of entry -> (respawn, routes,) precedence
    _run(sim)                                                   # (2) after enter_now()
    _open(sim, 'entry'); _on(sim, *OPEN)
    sim.enter_now(); _on(sim, 'opts', 'retire', 'scene')       # admit, by order of entry -> respawn, routes, precedence
    _open(sim, 'entry'); _on(sim, *OPEN)
    sim.enter_on_schedule(WAIT); _on(sim, 'opts', 'retire', 'scene', 'admit', 'precedence')    # replaces respawn and routes, keeps the order
    assert sim._precedence.mode == _lib.PRECEDENCE_ENTRY
    _open(sim, fixed); _on(sim, *OPEN)
    sim.enter_on_schedule(WAIT); _on(sim, 'opts', 'retire', 'scene', 'admit', 'precedence')    # ... in either mode
    _open(sim, fixed); _on(sim, *OPEN)
    assert sim._precedence.mode == _lib.PRECEDENCE_FIXED
    sim.enter_now(); _on(sim, 'opts', 'retire', 'scene', 'precedence')     # admit, fixed words -> respawn, routes
    sim.yield_to_everyone(); _on(sim, 'opts', 'retire', 'scene')           # precedence -> nothing
    _open(sim, fixed); _on(sim, *OPEN)
    sim.retire_at_goal(leave_scene=True); _on(sim, 'opts', 'retire', 'scene')      # replaces the scene and what lives on it: a new one
    _open(sim, fixed); _on(sim, *OPEN)
    sim.retire_at_goal(); _on(sim, 'opts', 'retire')           # ... and none: scene -> admit, respawn, routes, precedence
    _open(sim, 'entry'); _on(sim, *OPEN)
    sim.keep_driving(); _on(sim, 'opts')                        # retire -> scene, admit, respawn, routes, precedence
    # ---- the stages that live on the signals
    sim.signalise(plan); _on(sim, 'opts', 'signals')
    sim.advise_speed(); _on(sim, 'opts', 'signals', 'advice')
    _run(sim)                                                   # (3) signals + advice
    sim.share_plans(); _on(sim, 'opts', 'signals', 'advice', 'intent')
    sim.stop_advising(); _on(sim, 'opts', 'signals', 'intent')  # advice -> nothing
    sim.keep_plans_private(); _on(sim, 'opts', 'signals')      # intent -> nothing
    sim.advise_speed()
    sim.reserve(mgr); _on(sim, 'opts', 'signals', 'reservation')           # replaces (actuation and) advice
    _run(sim)                                                   # (4) after reserve()
    sim.actuate(ctrl); _on(sim, 'opts', 'signals', 'actuation')            # replaces (advice and) reservation
    sim.reserve(mgr); _on(sim, 'opts', 'signals', 'reservation')           # replaces actuation
    sim.actuate(ctrl)
    sim.signalise(plan); _on(sim, 'opts', 'signals')           # replaces actuation
    sim.advise_speed()
    sim.actuate(ctrl); _on(sim, 'opts', 'signals', 'actuation')            # replaces advice
    sim.unsignalise(); _on(sim, 'opts')                         # signals -> actuation
    sim.reserve(mgr)
    sim.advise_speed(); _on(sim, 'opts', 'signals', 'advice', 'reservation')       # (accepted here; run() refuses the pair)
    sim.signalise(plan); _on(sim, 'opts', 'signals', 'advice')             # replaces reservation, keeps advice
    sim.reserve(mgr)
    sim.advise_speed()
    sim.unsignalise(); _on(sim, 'opts')                         # signals -> reservation, advice
    # ---- the snapshot names the words of what is on, and of nothing else
    assert set(sim.snapshot()) == BASE_KEYS
    sim.signalise(plan); sim.advise_speed()
    assert set(sim.snapshot()) == BASE_KEYS | {'held', 'advised'}
    sim.actuate(ctrl)
    assert set(sim.snapshot()) == BASE_KEYS | {'held', 'phase', 'stage', 'lights'}
    sim.reserve(mgr); sim.share_plans(); _open(sim, 'entry')
    _on(sim, *OPEN, 'signals', 'intent', 'reservation')
    snap = sim.snapshot()
    assert set(snap) == BASE_KEYS | {'done', 'steps_driven', 'absent', 'wait', 'entered_step', 'served', 'route', 'precedence', 'held',
                                     'shared_frames', 'granted', 'since', 'occupied'}
    assert all(isinstance(v, np.ndarray) for v in snap.values()) and snap['route'].tolist() == list(range(8))
    assert snap['precedence'].dtype == snap['granted'].dtype == snap['done'].dtype == np.int32 and snap['precedence'].shape == (8,)
