"""GPU tests of RESPAWN in the device-resident closed loop (mpcx_closed_loop_run_respawn, IntersectionBatch.respawn_on_schedule): a departed
agent's slot is reset, on the device and as the last launch of the step, for the next vehicle of its stream and handed back to the admission
gate.  The defining properties: a respawned vehicle starts exactly like a fresh one (its log rows repeat the first vehicle's bit for bit), and
a run with device respawn equals, bit for bit, a run with admission alone whose words the host build of the rule (tests/respawn_ref) rewrites
between run(1) calls -- while every driving agent of every step equals the oracle step over the present rows.  Then: graph replay and
chunking, scripted traffic, off means off, the refusals, run_until_done and episodes().  The host build of the rule is
tests/test_respawn_cpu.py.

Run lengths, established on the CPU oracle alone (tests/respawn_helpers.RespawnOracleLoop, T = 13, v0 = 0, gap 1 m,
due = [[0, 10, 60], [5, 20, 30]]): the three instances of QUEUE3 finish their six episodes in 145 / 139 / 158 steps in cut mode and
130 / 149 / 180 steps in speed mode."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import torch

from tests import admit_helpers as AH
from tests import respawn_helpers as RH
from tests import test_gpu_scene as GS

pytestmark = pytest.mark.gpu

T = 13
ROUTE3 = [[0, 0], [0, 2], [2, 0]]
START3 = [[600, 600], [330, 300], [300, 330]]
DUE2 = [[0, 10, 60], [5, 20, 30]]
DUE3 = np.tile(np.array(DUE2), (3, 1, 1))
STEPS3 = 200
LOG_WORDS = ('steps', 'goal_step', 'contact_step', 'flags', 'min_clearance')


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def stock(ctx):
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    return stock_routes(ctx)


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp('respawn_ref')
    return types.SimpleNamespace(admit=AH.build_ref(d), respawn=RH.build_ref(d))


def _batch(c, stock, route, start, mode='cut', traffic=None):
    """agents on the stock routes `route` (B, A) from the indices `start`, v0 = 0, retire_at_goal(leave_scene=True)"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    routes, dl, cd = stock
    kw = {}
    params = MpcParams(T=T, L=cd.distance_back_to_front_wheel)
    if mode == 'speed':
        import mpc_for_av_at_intersection_amd.lib.mpc_with_speed as ws
        params = dataclasses.replace(ws.params(cd, 0.2), L=cd.distance_back_to_front_wheel)
        kw['stop_mode'] = 'speed'
    if traffic is not None:
        kw['traffic'] = traffic
    sim = IntersectionBatch(c, params, GS._ip(cd, dl), routes, dl, np.asarray(route), np.asarray(start), **kw)
    sim.retire_at_goal(leave_scene=True)
    return sim


def _words(sim):
    """name -> device tensor of every word the rule may write, under the names of respawn_helpers.Case"""
    t = dict(state=sim.state, applied=sim.applied, u=sim.sol['u'], traj_idx=sim.traj_idx, target_ind=sim.target_ind, cut_len=sim.inter['cut_len'],
             iters=sim.sol['iters'], steps_driven=sim.steps_driven, wait=sim.wait, entered=sim.entered_step)
    if sim.prev_len is not None:
        t['prev_len'] = sim.prev_len
    if sim.log is not None:
        t.update(lsteps=sim.log.steps, goal_step=sim.log.goal_step, contact_step=sim.log.contact_step, flags=sim.log.flags,
                 min_clearance=sim.log.min_clearance)
    return t


class HandDriven:
    """the twin: a batch with ADMISSION ONLY (enter_on_schedule with the first vehicles' due steps), and the host build of the respawn rule
    applied to its device words with torch copies after every run(1).  served and the episode table live on the host."""

    def __init__(self, libs, sim, due, gap):
        self.libs, self.sim = libs, sim
        due = np.asarray(due).reshape(sim.P, -1)
        self.case = RH.Case(sim.P, T, due.shape[1], int(sim.obs6.shape[0]), log=sim.log is not None, speed=sim.prev_len is not None,
                            start_state=sim.state.cpu().numpy(), start_idx=sim.traj_idx.cpu().numpy(), due=due, own=sim.obs_skip.cpu().numpy())
        sim.enter_on_schedule(due[:, 0], gap)
        assert sim._respawn is None and sim._admit is not None
        self.gap = float(gap)
        self.rows = {k: getattr(sim, k).cpu().numpy() for k in ('obs_off', 'obs_cnt', 'obs_skip')}

    def admitted(self, snap):
        """snap with done / absent as this step's admission stage WILL leave them (the host build of the admission rule on copies): whom
        the step drives and whom it sees"""
        sim = self.sim
        case = AH.Case(snap['state'], own=self.rows['obs_skip'], wait=snap['wait'].copy(), done=snap['done'].copy(), absent=snap['absent'].copy(),
                       gap=self.gap, radius=sim.ip.radius, centers=sim.ip.circle_centers, obs_off=self.rows['obs_off'], obs_cnt=self.rows['obs_cnt'],
                       clock=int(sim.clock.item()), entered=snap['entered_step'].copy())
        AH.host_step(self.libs.admit, case)
        snap = dict(snap)
        snap['done'], snap['absent'] = case.done.copy(), case.absent.copy()
        return snap, case

    def respawn(self):
        """this step's respawn on the host: the device words into the Case, the rule, the words back if somebody arrived"""
        sim, c = self.sim, self.case
        sim.ctx.synchronize()
        dev = _words(sim)
        for k, t in dev.items():
            getattr(c, k)[...] = t.cpu().numpy().reshape(getattr(c, k).shape)
        c.done[...] = sim.done.cpu().numpy()
        c.clock[...] = sim.clock.cpu().numpy()
        if RH.host_step(self.libs.respawn, c):
            for k, t in dev.items():
                t.copy_(torch.from_numpy(getattr(c, k).reshape(tuple(t.shape))).to(t.device))
            sim.ctx.synchronize()


def _pair_of_runs(ctx, libs, stock, route, start, due, gap, steps, mode='cut', log=0, replay=True, traffic=None, until_served=None):
    """X with respawn_on_schedule beside its hand-driven twin Y for `steps` steps of run(1) (or until X has served until_served episodes);
    after every step every snapshot key of Y must be X's bit for bit, as must wait, entered_step, served, the episode table and the log's
    outcome words; and (replay) every driving agent equals the oracle step over the present rows"""
    X = _batch(ctx, stock, route, start, mode, traffic() if traffic else None)
    Ysim = _batch(ctx, stock, route, start, mode, traffic() if traffic else None)
    if log:
        X.attach_log(log); Ysim.attach_log(log)
    X.respawn_on_schedule(due, gap=gap)
    Y = HandDriven(libs, Ysim, due, gap)
    worst, taken = 0.0, 0
    for s in range(steps):
        X.run(1)
        before = Ysim.snapshot()
        if replay:
            before, gate = Y.admitted(before)
        Ysim.run(1)
        after = Ysim.snapshot()
        if replay:
            assert np.array_equal(after['wait'], gate.wait) and np.array_equal(after['entered_step'], gate.entered), s
            w, _ = GS._replay_step(Ysim, before, after, GS._pool_before(Ysim, before, after), before['absent'])
            worst = max(worst, w)
        Y.respawn()
        x, y = X.snapshot(), Ysim.snapshot()
        assert sorted(x) == sorted(list(y) + ['served'])
        for k in y:
            assert x[k].tobytes() == y[k].tobytes(), (s, k)
        c = Y.case
        assert np.array_equal(x['served'], c.served) and int(X.clock.item()) == s + 1 == int(Ysim.clock.item()), s
        assert X.ep_i32.cpu().numpy().tobytes() == c.ep_i32.tobytes() and X.ep_f64.cpu().numpy().tobytes() == c.ep_f64.tobytes(), s
        if log:
            for k in LOG_WORDS:
                assert getattr(X.log, k).cpu().numpy().tobytes() == getattr(Ysim.log, k).cpu().numpy().tobytes(), (s, k)
        taken = s + 1
        if until_served is not None and int(x['served'].sum()) >= until_served:
            break
    if log:
        assert X.log.rows_f64.cpu().numpy().tobytes() == Ysim.log.rows_f64.cpu().numpy().tobytes()
        assert X.log.rows_i32.cpu().numpy().tobytes() == Ysim.log.rows_i32.cpu().numpy().tobytes()
    return types.SimpleNamespace(X=X, Y=Y, worst=worst, taken=taken)


# ---------------------------------------------------------------- G1
def test_stage_alone(ctx, libs):
    """G1.  Context.respawn_step on the hand-made words of tests/test_respawn_cpu.py -- with and without log words, with and without
    prev_len -- gives the words of the host build, word for word; so does a second step on the device's own words."""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    arrived = 0
    for log, speed in ((True, False), (False, False), (True, True), (False, True)):
        host = RH.hand_made(log, speed)
        ctx.set_mpc_params(MpcParams(T=host.T, L=2.86))
        names = RH.MUT_F64 + RH.MUT_I32 + RH.CONST_I32 + ('start_state',)
        dev = types.SimpleNamespace(G=host.G, log=log, **{k: torch.from_numpy(getattr(host, k).copy()).to(ctx.device) for k in names})
        for step in range(2):
            lg, retire, admit, rs = RH.structs(dev, ptr=lambda t: t.data_ptr())
            ctx.respawn_step(dev.state, dev.applied, dev.u.view(host.P, 2, host.T), dev.traj_idx, dev.target_ind, dev.cut_len, dev.iters, dev.own,
                             host.n_pool, retire, admit, rs, prev_len=dev.prev_len if speed else None, log=lg)
            ctx.synchronize()
            arrived += RH.host_step(libs.respawn, host)
            for k in RH.MUT_F64 + RH.MUT_I32:
                assert getattr(dev, k).cpu().numpy().tobytes() == getattr(host, k).tobytes(), (log, speed, step, k)
            host.clock[0] += 1
            dev.clock += 1
    assert arrived == 4 * len(RH.ARRIVE)


# ---------------------------------------------------------------- G2
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_a_respawned_vehicle_starts_like_a_fresh_one(ctx, stock, mode):
    """G2.  B = 2, A = 1: route (1, 1) from indices 600 and 640, G = 3, due all 0, gap 0, a log of 96 rows, 80 steps of run(1).  For each
    slot the log rows of episodes 1 and 2 equal those of episode 0 bit for bit, all 16 columns; steps_driven is equal across the three
    episodes and arrived - entered + 1 == steps_driven.  A word the reset forgot would show here."""
    sim = _batch(ctx, stock, [[0], [0]], [[600], [640]], mode)
    log = sim.attach_log(96)
    sim.respawn_on_schedule(np.zeros((2, 1, 3), dtype=np.int64), gap=0.0)
    for _ in range(80):
        sim.run(1)
    ep = sim.episodes()
    print(mode, ep)
    assert sim.served_count() == 6 and len(ep) == 6 and sim.snapshot()['served'].tolist() == [3, 3]
    assert ep['slot'].tolist() == [0, 0, 0, 1, 1, 1] and ep['generation'].tolist() == [0, 1, 2, 0, 1, 2]
    assert (ep['arrived'] - ep['entered'] + 1 == ep['steps_driven']).all() and (ep['row_end'] - ep['row_begin'] == ep['steps_driven']).all()
    f, w = log.rows_f64.cpu().numpy(), log.rows_i32.cpu().numpy()
    for q in range(2):
        e = ep[ep['slot'] == q]
        assert len(set(e['steps_driven'].tolist())) == 1 and e['steps_driven'][0] > 5, e
        assert e['entered'].tolist() == [0] + (e['arrived'][:2] + 1).tolist() and e['row_begin'].tolist() == [0] + e['row_end'][:2].tolist()
        first = slice(e['row_begin'][0], e['row_end'][0])
        for g in (1, 2):
            rows = slice(e['row_begin'][g], e['row_end'][g])
            assert f[rows, q].tobytes() == f[first, q].tobytes() and w[rows, q].tobytes() == w[first, q].tobytes(), (q, g)
    assert not ep['contact'].any() and np.isinf(ep['min_clearance']).all()          # nobody else in the scene
    assert ep['steps_driven'][0] == (25 if mode == 'cut' else 23)                    # the CPU oracle's (tests/test_respawn_cpu.py)


# ---------------------------------------------------------------- G3
@pytest.fixture(scope='module', params=['cut', 'speed'])
def twins(request, ctx, libs, stock):
    return request.param, _pair_of_runs(ctx, libs, stock, ROUTE3, START3, DUE3, 1.0, STEPS3, mode=request.param, log=192)


def test_device_respawn_equals_a_hand_driven_twin(twins):
    """G3.  B = 3, A = 2, two slots per instance, three vehicles per slot, gap 1 m, 200 steps, both stop modes: after every step every
    snapshot key, wait, entered_step, served, the episode table and the log's words of the device run equal those of the twin that has
    admission only and whose words the host build of the rule rewrites between steps; every driving agent of every step equals the oracle
    step over the present rows within 2e-7 -- all asserted while the fixture ran.  All 18 episodes are finished when the run ends (on the
    CPU oracle the instances finish in 145 / 139 / 158 steps in cut mode and 130 / 149 / 180 in speed mode)."""
    mode, r = twins
    ep = r.X.episodes()
    print('%s: worst |GPU - oracle| %.2e over %d steps; last arrival per instance %s' %
          (mode, r.worst, r.taken, [int(ep['arrived'][ep['slot'] // 2 == b].max()) + 1 for b in range(3)]))
    assert r.X.served_count() == 18 and len(ep) == 18 and r.X.snapshot()['served'].tolist() == [3] * 6
    assert (ep['arrived'] - ep['entered'] + 1 == ep['steps_driven']).all() and (ep['delay'] >= 0).all()
    assert (ep['due'].reshape(6, 3) == DUE3.reshape(6, 3)).all()
    want = [145, 139, 158] if mode == 'cut' else [130, 149, 180]
    assert [int(ep['arrived'][ep['slot'] // 2 == b].max()) + 1 for b in range(3)] == want
    if mode == 'cut':       # instance 0 is the queue of tests/test_respawn_cpu.py
        got = [[tuple(int(e[k]) for k in ('entered', 'arrived', 'steps_driven')) for e in ep[ep['slot'] == q]] for q in range(2)]
        assert got == [[(0, 24, 25), (37, 72, 36), (85, 120, 36)], [(13, 48, 36), (61, 96, 36), (109, 144, 36)]], got


# ---------------------------------------------------------------- G4
def test_graph_replay_and_chunking(ctx, stock):
    """G4.  G3's batch as 29 chunks of run(7, graph=True) equals 203 x run(1) plain, in the final snapshot and in episodes()."""
    from mpc_for_av_at_intersection_amd.runtime import Context

    def fresh(c):
        sim = _batch(c, stock, ROUTE3, START3)
        sim.respawn_on_schedule(DUE3, gap=1.0)
        return sim
    plain = fresh(ctx)
    for _ in range(203):
        plain.run(1)
    a = plain.snapshot()
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = fresh(side)
        torch.cuda.synchronize()
        for _ in range(29):
            graph.run(7, graph=True)
        b = graph.snapshot()
        assert sorted(a) == sorted(b) and 'served' in a
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert int(graph.clock.item()) == 203 == int(plain.clock.item())
        assert plain.episodes().tobytes() == graph.episodes().tobytes() and len(plain.episodes()) == 18
    finally:
        side.close()


# ---------------------------------------------------------------- G5
def test_scripted_traffic(ctx, libs, stock):
    """G5.  One instance of the stock scenario: the ego on its stock route and the stock pair of scripted cars, the second of which spawns
    on the ego's start pose; the ego respawns once (G = 2), gap 1 m.  Twin equality after every step as in G3, traffic_state and the pool
    included, until both episodes are finished."""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_specs
    routes, dl, cd = stock
    traffic = lambda: scripted_traffic_specs(1, 2, 0, cd.distance_back_to_front_wheel, dt=0.2)
    r = _pair_of_runs(ctx, libs, stock, [[6]], [[0]], np.zeros((1, 1, 2), dtype=np.int64), 1.0, 400, replay=False, traffic=traffic, until_served=2)
    ep = r.X.episodes()
    print('scripted traffic:', ep, 'in', r.taken, 'steps')
    assert r.X.served_count() == 2 and 'traffic_state' in r.X.snapshot()
    assert ep['entered'][0] > 20 and ep['entered'][1] == ep['arrived'][0] + 1           # held back by the standing car; the road is free later
    assert (ep['arrived'] - ep['entered'] + 1 == ep['steps_driven']).all()


# ---------------------------------------------------------------- G6
def _entry(sim, respawn, n, admit='own', retire='own', scene='own'):
    """mpcx_closed_loop_run_respawn itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    pick = lambda v, own: own if isinstance(v, str) else v
    ad, re_, sc = pick(admit, sim._admit), pick(retire, sim._retire), pick(scene, sim._scene)
    ref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_respawn(c._ctx, C.byref(cip), C.byref(sim._desc), None, ref(sim._opts), ref(re_), ref(sc), ref(ad), ref(respawn),
                                              int(n), 0))


def test_off_means_off(ctx, stock):
    """G6a.  respawn = NULL, an all-zero struct and stop_respawning() each give snapshots bit-identical to the admission-only run -- 40
    steps of G3's first instance, the first arrival (step 24) included: without respawn the slot stays empty."""
    from mpc_for_av_at_intersection_amd import _lib
    due = np.array([DUE2])

    def fresh():
        sim = _batch(ctx, stock, ROUTE3[:1], START3[:1])
        sim.enter_on_schedule(due[..., 0], gap=1.0)
        return sim
    base = fresh()
    base.run(40)
    want = base.snapshot()
    assert want['done'].tolist() == [1, 0] and want['steps_driven'].tolist() == [25, 27] and 'served' not in want
    runs = {}
    sim = fresh(); _entry(sim, None, 40); runs['NULL'] = sim.snapshot()
    sim = fresh(); _entry(sim, _lib.RespawnC(), 40); runs['zero struct'] = sim.snapshot()
    sim = _batch(ctx, stock, ROUTE3[:1], START3[:1])
    sim.respawn_on_schedule(due, gap=1.0)
    sim.stop_respawning()
    assert sim._respawn is None and sim._admit is not None
    sim.run(40)
    runs['stop_respawning'] = sim.snapshot()
    assert sim.served_count() == 0
    for name, got in runs.items():
        assert sorted(got) == sorted(want), name
        for k in want:
            assert want[k].tobytes() == got[k].tobytes(), (name, k)


def test_refusals(ctx, stock):
    """G6b.  MPCX_E_INVALID with a "respawn: ..." message before anything is launched, whatever n_steps is: respawn without admission (with
    or without the scene and retirement below it), generations < 1, each of the six pointers missing.  In Python: respawn_on_schedule
    without retire_at_goal(leave_scene=True), a bad due array.  keep_driving() and enter_now() switch respawn off."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _batch(ctx, stock, ROUTE3[:1], START3[:1])
    sim.respawn_on_schedule([DUE2], gap=1.0)
    before = sim.snapshot()
    rs = sim._respawn
    good = [rs.generations, 0, rs.start_state, rs.start_idx, rs.due, rs.served, rs.ep_i32, rs.ep_f64]
    for n in (0, 3):
        with pytest.raises(MpcxError, match='respawn: respawn needs admission'):
            _entry(sim, rs, n, admit=None)
        with pytest.raises(MpcxError, match='respawn: respawn needs admission'):
            _entry(sim, rs, n, admit=None, scene=None, retire=None)
        for g in (0, -1):
            with pytest.raises(MpcxError, match='respawn: generations'):
                _entry(sim, _lib.RespawnC(g, *good[1:]), n)
        for i, name in enumerate(('start_state', 'start_idx', 'due', 'served', 'ep_i32', 'ep_f64')):
            bad = list(good); bad[2 + i] = None
            with pytest.raises(MpcxError, match='respawn: .*%s is null' % name):
                _entry(sim, _lib.RespawnC(*bad), n)
    after = sim.snapshot()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert int(sim.clock.item()) == 0 and sim.served_count() == 0
    with pytest.raises(ValueError):
        sim.respawn_on_schedule([[0, 1, 2]])
    with pytest.raises(ValueError):
        sim.respawn_on_schedule(np.zeros((1, 2, 3)))
    with pytest.raises(ValueError):
        sim.respawn_on_schedule([[[0, -1], [0, 1]]])
    plain = GS._pair(ctx, stock, backs=(20.0,), leave=False)
    with pytest.raises(MpcxError, match='retire_at_goal\\(leave_scene=True\\)'):
        plain.respawn_on_schedule(np.zeros((1, 2, 2), dtype=np.int64))
    for off in ('enter_now', 'keep_driving'):
        sim = _batch(ctx, stock, ROUTE3[:1], START3[:1])
        sim.respawn_on_schedule([DUE2], gap=1.0)
        assert 'served' in sim.snapshot()
        getattr(sim, off)()
        assert sim._respawn is None and sim._admit is None and 'served' not in sim.snapshot()


# ---------------------------------------------------------------- G7
def test_run_until_done_and_episodes(ctx, stock, twins):
    """G7.  G3's batch under run_until_done: it goes on while a reset slot waits and ends once every slot is finished, with served_count()
    == P G; episodes() has exactly that many rows, delays are entered - due >= 0, row_end - row_begin == steps_driven, and the table is
    that of the stepped run."""
    mode, r = twins
    sim = _batch(ctx, stock, ROUTE3, START3, mode)
    sim.attach_log(192)
    sim.respawn_on_schedule(DUE3, gap=1.0)
    taken = sim.run_until_done(400, chunk=16)
    assert sim.served_count() == 18 == sim.P * 3 and sim.active_count() == 0 and sim.waiting_count() == 0 and taken < 400
    ep = sim.episodes()
    assert len(ep) == 18 and (ep['delay'] == ep['entered'] - ep['due']).all() and (ep['delay'] >= 0).all()
    assert (ep['row_end'] - ep['row_begin'] == ep['steps_driven']).all() and (ep['row_begin'] >= 0).all()
    assert ep.tobytes() == r.X.episodes().tobytes()
    assert len(sim.log.rows(0)) == ep['row_end'][ep['slot'] == 0].max()
