"""The composed oracle of the whole stack (tests/stack_helpers.py) without a GPU.  (1) With one rule on at a time StackOracleLoop reproduces
the rule-specific oracle loops step for step, byte for byte in every word they share: the composition adds nothing of its own.  (2) The scenes
of tests/test_gpu_stack.py, run free on the CPU, contain every event the GPU tests claim to cover."""
import numpy as np
import pytest

from tests import follow_helpers as FH
from tests import helpers as H
from tests import intent_helpers as IH
from tests import precedence_helpers as PH
from tests import reserve_helpers as RV
from tests import route_helpers as TH
from tests import stack_helpers as K


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    return K.build_libs(tmp_path_factory.mktemp('stack_ref'))


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a, b)


def _shared(loop, mine, out, s, speed):
    """the words every oracle loop has, against the stack's after the same step"""
    w = mine.words
    A = loop.A
    _same(loop.state, w['state'], (s, 'state')); _same(loop.applied, w['applied'], (s, 'applied'))
    _same(np.array(loop.traj_idx, np.int32), w['traj_idx'], (s, 'traj_idx')); _same(np.array(loop.target, np.int32), w['target_ind'], (s, 'target'))
    _same(np.array(loop.prev, np.int32), w['prev_len' if speed else 'cut_len'], (s, 'prev'))
    _same(np.array(loop.done, np.int32), w['done'], (s, 'done')); _same(np.array(loop.absent, np.int32), w['absent'][:A], (s, 'absent'))
    for a in range(A):
        _same(np.zeros((2, mine.cfg.T)) if loop.u[a] is None else loop.u[a], w['u'][a], (s, a, 'u'))
        if out[a] is not None and not ('served' in w and a in mine.last['arrived']):        # (a slot that was reset holds its next vehicle's words)
            cut = len(mine.last['agents'][a]['full']) if speed and out[a]['cut'] == 999 else out[a]['cut']
            assert (cut, out[a]['hit'], out[a]['status']) == (w['cut_len'][a], w['hit_idx'][a], w['status'][a]), (s, a)
            _same(out[a]['x_sol'], w['x'][a], (s, a, 'x'))


@pytest.mark.parametrize('speed', [False, True])
def test_equals_the_route_loop(libs, speed):
    """admission, retirement with departure and respawn with routes alone: RouteOracleLoop, two slots of one arm near the end of their
    routes, three vehicles each on alternating routes, gap 1 m, 40 steps in which both slots are reset and re-admitted on the other route"""
    routes = [H.smoothed_path(1, 1), H.smoothed_path(1, 2)]
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    route_of = [[0, 1, 0], [1, 0, 1]]
    start = [[len(routes[r]) - 120 - 90 * a for r in row] for a, row in enumerate(route_of)]
    due = [[0, 0, 0], [0, 0, 30]]
    loop = TH.RouteOracleLoop(libs.admit, libs.route, routes, dl, route_of, start, due, 1.0, T=13, speed=speed)
    cfg = K.make_config(libs, routes, dl, 1, 2, speed=speed, gap=1.0, due=[due], route_of=[route_of], start_idx=[start])
    mine = K.StackOracleLoop(cfg, K.initial_words(cfg, None, None))
    for s in range(40):
        out = loop.step(); mine.step()
        _shared(loop, mine, out, s, speed)
        w = mine.words
        for k, v in (('wait', loop.wait), ('entered_step', loop.entered), ('clock', loop.clock), ('served', loop.served), ('ep_i32', loop.ep_i32),
                     ('ep_f64', loop.ep_f64), ('steps_driven', loop.steps_driven), ('path_off', loop.path_off), ('path_len', loop.path_len)):
            _same(v, w[k], (s, k))
    assert loop.served.tolist() == [1, 1] and mine.events['new_route'] == 2 and w['path_off'].tolist() == [int(cfg.route_off[1]), 0]


def test_equals_the_precedence_loop(libs):
    """right of way alone, fixed words: PrecedenceOracleLoop on the scene 'eight', 30 steps"""
    pairs, start = PH.scene('eight')
    routes = [H.smoothed_path(*pr) for pr in pairs]
    loop = PH.scene_loop('eight')
    cfg = K.make_config(libs, routes, loop.dl, 1, 8, precedence='fixed')
    mine = K.StackOracleLoop(cfg, K.initial_words(cfg, np.arange(8), start, prec=np.arange(8)))
    for s in range(30):
        out = loop.step(); mine.step()
        _shared(loop, mine, out, s, False)
    assert sum(o['hit'] >= 0 for o in out if o is not None) > 0


def test_equals_the_reserve_loop(libs):
    """a reservation manager alone: ReserveOracleLoop.scene_loop('eight', patience 0), 40 steps"""
    loop = RV.scene_loop('eight', 0)
    paths, dl, start, stop, group, ex, conflict, lane = RV.scene_tables('eight')
    detect = max(int(s[0]) for s in stop)
    cfg = K.make_config(libs, paths, dl, 1, 8, reserve=dict(managers=[(detect, 0)], stop=np.concatenate(stop), group=np.concatenate(group),
                                                           exit=np.concatenate(ex), conflict=conflict, lane=lane))
    mine = K.StackOracleLoop(cfg, K.initial_words(cfg, np.arange(8), start))
    for s in range(40):
        out = loop.step(); mine.step()
        _shared(loop, mine, out, s, False)
        w = mine.words
        for k, v in (('held', np.array(loop.held, np.int32)), ('granted', loop.grant), ('since', loop.since), ('junction_clock', loop.clock),
                     ('occupied', np.array(loop.occupied_hist[-1:], np.int32)), ('queued', np.array(loop.queued_hist[-1:], np.int32))):
            _same(v, w[k], (s, k))
    assert mine.events['granted'] == len(loop.grants) > 0 and mine.events['refused_by_grant'] > 0


@pytest.mark.parametrize('speed', [False, True])
def test_equals_the_follow_loop(libs, speed):
    """following beside a fixed plan: FollowOracleLoop.queue_loop, 40 steps in both modes"""
    loop = FH.queue_loop(speed)
    paths, dl, start, stop, group = FH.queue_scene(5)
    cfg = K.make_config(libs, paths[:1], dl, 1, 5, speed=speed, signals=dict(plans=[loop.plan], stop=stop[0], group=group[0], brake=loop.brake),
                        follow=FH.FOLLOW)
    mine = K.StackOracleLoop(cfg, K.initial_words(cfg, np.zeros(5), start))
    led = 0
    for s in range(40):
        out = loop.step(); mine.step()
        _shared(loop, mine, out, s, speed)
        w = mine.words
        _same(np.array(loop.held, np.int32), w['held'], (s, 'held')); _same(np.array(loop.tick, np.int32), w['tick'], (s, 'tick'))
        for a in range(5):
            assert out[a]['leader'] == w['leader'][a] and np.float64(out[a]['gap']).tobytes() == w['gap'][a].tobytes(), (s, a)
            assert np.float64(out[a]['cap']).tobytes() == w['follow_cap'][a].tobytes(), (s, a)
            led += out[a]['leader'] >= 0
    assert led == 160


def test_equals_the_intent_loop(libs):
    """shared plans beside a fixed plan: IntentOracleLoop on red_light_scene (speed mode from cruise speed), 40 steps"""
    from mpc_for_av_at_intersection_amd.batch import stop_lines, two_phase_plan
    from tests import signal_helpers as G
    from tests import speedref_helpers as S
    from tests.test_intent_cpu import RED_LIGHT
    plan = two_phase_plan(**G.PLAN)
    loop = IH.red_light_scene(RED_LIGHT['held_start'], RED_LIGHT['green_start'], [True, True], S.V_REF, plan, tick=RED_LIGHT['tick'])
    paths = [H.smoothed_path(1, 2), H.smoothed_path(2, 2)]
    stop, group = stop_lines(paths)
    cfg = K.make_config(libs, paths, loop.dl, 1, 2, speed=True, signals=dict(plans=[plan], stop=stop, group=group, brake=loop.brake), share=[1, 1])
    words = K.initial_words(cfg, [0, 1], [RED_LIGHT['held_start'], RED_LIGHT['green_start']], tick=[RED_LIGHT['tick']] * 2)
    words['state'][:, 2] = S.V_REF
    mine = K.StackOracleLoop(cfg, words)
    shared = 0
    for s in range(40):
        out = loop.step(); mine.step()
        _shared(loop, mine, out, s, True)
        w = mine.words
        _same(np.array(loop.held, np.int32), w['held'], (s, 'held'))
        for a in range(2):
            if out[a] is not None:
                assert out[a]['shared'] == bool(w['shared_frames'][a]), (s, a)
                shared += out[a]['shared']
    assert shared > 40 and sum(len(h) for h in loop.hit_steps) > 0


@pytest.fixture(scope='module')
def stock():
    return K.stock_paths()


@pytest.mark.parametrize('kind,speed', [('plan', False), ('plan', True), ('reserve', False), ('reserve', True)])
def test_scenes_contain_their_events(libs, stock, kind, speed):
    """The scenes of tests/test_gpu_stack.py K1 ('plan') and K2 ('reserve'), run free on the CPU for stack_helpers.STEPS steps, contain every
    event of stack_helpers.REQUIRED, and every instance completes an episode whose record carries the log's outcome words.  Counts of the
    free run (agent-steps, or vehicles for the first four):
      K1 cut:    new_route 9, ended_held 12, ended_leading 8, leader_yields 364, leader_shares 338, follow_cut_while_held 332,
                 hold_cut_with_leader 2, stand_and_plan 647, episodes 8 + 9
      K1 speed:  new_route 8, ended_held 0, ended_leading 10, leader_yields 344, leader_shares 241, follow_cut_while_held 241,
                 hold_cut_with_leader 3, stand_and_plan 630, cap_lowered 311, advice_lowered 800, episodes 8 + 8
      K2 cut:    new_route 9, ended_leading 8, ended_granted 0, leader_yields 365, leader_shares 302, follow_cut_while_held 114,
                 hold_cut_with_leader 4, stand_and_plan 567, refused_by_grant 347, granted 4, episodes 8 + 9
      K2 speed:  new_route 8, ended_leading 8, ended_granted 0, leader_yields 271, leader_shares 256, follow_cut_while_held 63,
                 hold_cut_with_leader 12, stand_and_plan 530, cap_lowered 270, refused_by_grant 302, granted 3, episodes 8 + 8
    ended_held in speed mode and ended_granted cannot occur in these scenes: stack_helpers.REQUIRED says why."""
    paths, dl = stock
    cfg, words, _ = K.scene_config(libs, kind, speed, paths, dl)
    loop = K.StackOracleLoop(cfg, words)
    ev = loop.run(K.STEPS[kind])
    print('%s, %s mode, %d steps: %s, episodes per instance %s' % (kind, 'speed' if speed else 'cut', loop.steps, ev, loop.episodes_of.tolist()))
    for name in K.REQUIRED[kind, speed]:
        assert ev[name] > 0, (name, ev)
    assert (loop.episodes_of > 0).all()
    w = loop.words
    fin = np.arange(cfg.respawn['G'])[None, :] < w['served'][:, None]
    assert (w['ep_i32'][fin][:, 3] >= w['ep_i32'][fin][:, 2]).all() and (w['ep_i32'][fin][:, 2] > 0).all()      # the log's cursor: a row per step driven
    assert np.isfinite(w['ep_f64'][fin][:, 0]).any() and (w['ep_i32'][fin][:, 5] & 1).any()                     # its clearance words
    if kind == 'reserve':       # both managers are met: strict first come first served refuses where the unbounded one grants
        assert w['junction_clock'].tolist() == [loop.steps] * 2


def test_queue_with_two_passes(libs, stock):
    """K4 on the CPU: 20 steps of the queue in speed mode with two linearisation passes.  The followers have leaders, the cap lowers windows,
    and the second pass matters: the run with one pass differs."""
    paths, dl = stock
    runs = []
    for passes in (2, 1):
        cfg, words = K.queue_config(libs, paths, dl, lin_passes=passes)
        loop = K.StackOracleLoop(cfg, words)
        loop.run(20)
        runs.append(loop)
    two, one = runs
    led = int((two.words['leader'] >= 0).sum())
    print('queue, two passes: %d agents led in the last step, %d windows capped; |u(2 passes) - u(1 pass)| %.3f'
          % (led, two.events['cap_lowered'], np.abs(two.words['u'] - one.words['u']).max()))
    assert led == 6 and two.events['cap_lowered'] > 0 and np.abs(two.words['u'] - one.words['u']).max() > 1e-3
