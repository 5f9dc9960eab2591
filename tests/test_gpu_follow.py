"""GPU tests of CAR FOLLOWING in the device-resident closed loop (mpcx_set_following, IntersectionBatch.follow): one launch in front of the
window stage finds every agent's leader on its own path and lowers its cut length (its stop index in speed mode) to a stop point behind it;
in speed mode one more behind the window stage caps its speed reference.  The stage entries equal the host build of the rule byte for
byte; every driving agent of every closed-loop step equals the oracle step under the rule (follow_helpers.follow_agent_step), beside
signals and advice, beside retirement and departure, and with a scripted actor in the pool; graph replay, off means off, the refusals, a
changed struct under graph replay.  B = 2, A = 4, T = 13, v0 = 0."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import advise_helpers as AH
from tests import follow_helpers as FH
from tests import scene_helpers as SH
from tests import signal_helpers as G
from tests import test_gpu_respawn as GR
from tests import test_gpu_scene as GS
from tests import test_gpu_signal as TS

pytestmark = pytest.mark.gpu

KEYS = GS.KEYS
QUEUE_ROUTE = 1                                             # the straight stock route from the south
QUEUE_START = np.array([[400, 300, 200, 100], [420, 330, 240, 150]])
OFFSET = np.array([60, 75])                                 # the clocks of the two instances: 40 and 25 steps of red left
# a standstill wider than the 10.3 m at which the conflict search stops a follower by itself, so that the rule's stop point is the shorter one
WIDE = dict(standstill=12.0, time_gap=1.5)
STEPS = 40


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
def ref(tmp_path_factory):
    return FH.build_ref(tmp_path_factory.mktemp('follow_ref'))


def _queue(c, stock, mode, signals=True, advise=False, follow=WIDE, retire=True, start=QUEUE_START, traffic=None):
    """B = 2 instances of four cars on one straight route, the first nearest a stop line at point follow_helpers.QUEUE_LINE of the route"""
    from mpc_for_av_at_intersection_amd.batch import stop_lines
    routes = stock[0]
    sim = GR._batch(c, stock, np.full((2, 4), QUEUE_ROUTE), np.asarray(start), mode, traffic=traffic)
    if not retire:
        sim.keep_driving()
    if signals:
        stop, group = stop_lines(routes)
        o = int(sum(len(r) for r in routes[:QUEUE_ROUTE]))
        L = len(routes[QUEUE_ROUTE])
        stop[o:o + L] = np.where(np.arange(L) <= FH.QUEUE_LINE, FH.QUEUE_LINE, -1)
        group[o:o + L] = 0
        sim.signalise(TS._plans(G.PLAN), stop=stop, group=group, offset=OFFSET)
        if advise:
            sim.advise_speed()
    if follow is not None:
        sim.follow(**follow)
    return sim


_snap = TS._snap


def _params(sim):
    f = sim._following
    return {n: getattr(f, n) for n in FH.PAR + ('reach',)}


def _replay_step(sim, before, after, pool, absent):
    """Every DRIVING agent of the step replayed on the oracle under the rule (follow_helpers.follow_agent_step), beside the signal hold and
    the advice where the batch has them.  traj_idx, cut_len, hit_idx, target_ind, status, held and leader identical; gap, cap and advised
    bitwise; row 2 of xref equal in speed mode; u and x within 2e-7 (the project's bar).  A retired agent's buffers are unchanged and it
    has no leader.  Returns (worst difference, agents with a leader, agents whose stop point was the shorter cut, whose window the cap lowered)."""
    from oracle import oracle_py as orc
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    speed = sim.stop_mode == 'speed'
    par = _params(sim)
    tabs = TS._tables(sim) if sim._signals is not None else None
    adv = None if sim._advice is None else dict(v_cruise=float(sim._advice.v_cruise), v_min=float(sim._advice.v_min),
                                                reach=float(sim._advice.reach), lead=int(sim._advice.lead))
    done = before['done'] if 'done' in before else np.zeros(sim.P, np.int32)
    worst, n_lead, n_cut, n_cap = 0.0, 0, 0, 0
    for p in range(sim.P):
        if done[p]:
            for k in KEYS:
                if k != 'applied':
                    assert before[k][p].tobytes() == after[k][p].tobytes(), (p, k)
            assert after['leader'][p] == -1 and after['gap'][p] == -1.0 and after['follow_cap'][p] == 0.0, p
            continue
        path = tab[off[p]:off[p] + ln[p]]
        slots = FH.others_of(int(o_off[p]), int(o_cnt[p]), int(o_skip[p]), len(pool), absent)
        present = [r for r in slots if r is not None]
        seen = {}

        def follow(ti, v, p=p, path=path, slots=slots, seen=seen):
            best = FH.leader_of(path, ti, pool, slots, par, par['reach'])
            if best is None:
                return None
            gap, s, cap = FH.stop_and_cap(ti, best[1], best[2], v, sim.dl, speed, par)
            seen['s'] = s
            return best[0], gap, s, cap

        decide = advise = None
        if tabs is not None:
            plan = int(tabs['plan_of'][p]); cycle = int(tabs['plan_cycle'][plan]); t = int(before['tick'][p]) % cycle

            def line(ti, p=p):
                i = int(off[p]) + ti
                return int(tabs['path_stop'][i]), int(tabs['path_group'][i])

            def decide(ti, v, p=p, plan=plan, cycle=cycle, t=t):
                s, g = line(ti)
                if s < 0 or ti >= s or s >= ln[p]:
                    return 0, s
                lt = G.light(cycle, int(tabs['plan_amber'][plan]), int(tabs['plan_green'][plan, g, 0]), int(tabs['plan_green'][plan, g, 1]), t)
                if lt == G.RED:
                    return 1, s
                if lt == G.AMBER and (before['held'][p] != 0 or np.float64(s - ti) * np.float64(sim.dl) >= np.float64(v) * np.float64(v) / (2.0 * tabs['brake'])):
                    return 2, s
                return 0, s

            if adv is not None:
                def advise(ti, cut, p=p, plan=plan, cycle=cycle, t=t):
                    s, g = line(ti)
                    if s < 0 or ti >= s or s >= ln[p] or cut < s:
                        return 0.0
                    return AH.advised_speed(ti, s, (t + 1) % cycle, cycle, int(tabs['plan_green'][plan, g, 0]), int(tabs['plan_green'][plan, g, 1]),
                                            sim.dl, float(sim.params.dt), **adv)
        kw = dict(v_ref=sim.v_ref) if speed else {}
        r = FH.follow_agent_step(po, path, sim.dl, before['state'][p], pool[present], int(before['traj_idx'][p]), int(before['prev_cut'][p]),
                                 int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius, sim.ip.cutoff_margin, speed, follow, decide,
                                 advise, **kw)
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        want_cut = int(ln[p]) if speed and r['cut'] == 999 else r['cut']
        want = (r['traj_idx'], want_cut, r['target_ind'], want_hit, r['sol'].status, r['leader'])
        got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['leader'][p])
        assert want == tuple(int(v) for v in got), (p, want, got)
        if tabs is not None:
            assert r['held'] == after['held'][p], p
        assert r['sol'].status == 0
        assert np.float64(r['gap']).tobytes() == after['gap'][p].tobytes() and np.float64(r['cap']).tobytes() == after['follow_cap'][p].tobytes(), \
            (p, r['gap'], after['gap'][p], r['cap'], after['follow_cap'][p])
        if adv is not None:
            assert np.float64(r['advised']).tobytes() == after['advised'][p].tobytes(), p
        if speed:
            assert np.array_equal(np.asarray(r['xref'])[2], after['xref'][p, 2]), (p, r['xref'][2], after['xref'][p, 2])
            n_cap += bool(r['cap'] > 0 and (np.asarray(r['xref'])[2] < np.minimum(np.asarray(r['xref_free'])[2], r['advised'] or np.inf)).any())
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        n_lead += r['leader'] >= 0
        n_cut += bool(r['leader'] >= 0 and seen['s'] == r['cut'])
        if 'done' in after:
            arrived = SH.is_goal(after['state'][p], path[-1], after['target_ind'][p], ln[p] if speed else after['cut_len'][p])
            assert bool(after['done'][p]) == arrived and after['absent'][o_skip[p]] == int(arrived), (p, arrived)
    assert worst < 2e-7, worst
    return worst, n_lead, n_cut, n_cap


def _stepped(sim, steps):
    tot = np.zeros(4)
    for s in range(steps):
        before = _snap(sim)
        sim.run(1)
        after = _snap(sim)
        absent = before['absent'] if 'absent' in before else np.zeros(int(sim.obs6.shape[0]), np.int32)
        w = _replay_step(sim, before, after, GS._pool_before(sim, before, after), absent)
        tot = np.array([max(tot[0], w[0]), tot[1] + w[1], tot[2] + w[2], tot[3] + w[3]])
    return tot, after


# ---------------------------------------------------------------- G1: the stage entries against the host build
def _device_stage(ctx, w):
    """both stage entries on the words w (a dict of follow_helpers.words()); returns the words the device leaves"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    P, _, W = w['xref'].shape
    if ctx.params is None or ctx.params.T != W - 1:
        ctx.set_mpc_params(MpcParams(T=W - 1))
    i32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.int32, device=ctx.device)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=ctx.device)
    d = {k: i32(w[k]) for k in FH.I32_KEYS + FH.OPT_KEYS}
    d.update({k: f64(w[k]) for k in FH.F64_KEYS + ('xref',)})
    out = dict(leader=torch.full((P,), -7, dtype=torch.int32, device=ctx.device), gap=torch.full((P,), float('nan'), dtype=torch.float64, device=ctx.device),
               cap=torch.full((P,), float('nan'), dtype=torch.float64, device=ctx.device))
    fl = _lib.FollowingC(out['leader'].data_ptr(), out['gap'].data_ptr(), out['cap'].data_ptr(), *[float(w[n]) for n in FH.PAR], w['reach'], P, 0)
    ctx.follow_step(float(w['dl']), _lib.STOP_SPEED if w['speed'] else _lib.STOP_CUT, d['state'], d['path'], d['path_off'], d['path_len'],
                    d['traj_idx'], d['cut_len'], d['obs6'], d['obs_off'], d['obs_cnt'], fl, obs_skip=d['obs_skip'], done=d['done'], absent=d['absent'])
    ctx.follow_cap_step(fl, d['xref'], done=d['done'])
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update({k: (None if d[k] is None else d[k].cpu().numpy()) for k in d})
    return got


def _same_as_host(ctx, ref, w, what):
    host = FH.copy_words(w)
    n = FH.host_rule(ref, host)
    FH.host_clamp(ref, host)
    got = _device_stage(ctx, w)
    for k in FH.OUT_KEYS + ('xref',):       # integers, gap and cap byte for byte (the device's double sqrt is correctly rounded)
        assert got[k].tobytes() == host[k].tobytes(), (what, k, np.flatnonzero(got[k].ravel() != host[k].ravel())[:8])
    for k in FH.I32_KEYS + FH.OPT_KEYS + FH.F64_KEYS:       # nothing else is written
        if k != 'cut_len' and w[k] is not None:
            assert got[k].tobytes() == w[k].tobytes(), (what, k)
    return n


@pytest.mark.parametrize('speed', [0, 1])
def test_stage_entries_on_hand_made_words(ctx, ref, speed):
    """G1a.  mpcx_follow_step_batch and mpcx_follow_cap_step_batch on the hand-made words of tests/test_follow_cpu.py, reach 20 and reach 1:
    leader, cut_len, gap, cap and xref equal the host build's, byte for byte, and nothing else is written"""
    for reach, leaders in ((20, 12), (1, 1)):
        w, _ = FH.hand_made(speed, reach=reach)
        assert _same_as_host(ctx, ref, w, reach) == leaders


@pytest.mark.parametrize('P', [1, 3, 5, 17, 67])
def test_stage_entries_on_random_scenes(ctx, ref, P):
    """G1b.  Seeded random scenes of P agents with 0..19 others each, so that lane groups straddle wavefronts and blocks and the last one
    is ragged: four seeds per P, both stop modes, with and without the optional words.  The same bytes as the host build."""
    leaders = 0
    for seed in range(4):
        leaders += _same_as_host(ctx, ref, FH.random_words(1000 + 16 * P + seed, P=P, W=(2, 6, 14, 33)[seed]), (P, seed))
    assert leaders > 0 or P == 1


# ---------------------------------------------------------------- G2: the closed loop on the oracle
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_queue_beside_signals_and_advice(ctx, stock, mode):
    """G2a.  The queue of tests/test_follow_cpu.py as 2 x 4 agents under signal_helpers.PLAN (red for another 40 and 25 steps), in speed mode
    with advice as well, standstill 12 m and time gap 1.5 s, 40 steps.  Every driving agent of every step equals the oracle step; not
    vacuous: agents have leaders, the rule's stop point is the shorter cut, and in speed mode its cap lowers windows."""
    sim = _queue(ctx, stock, mode, advise=mode == 'speed')
    (worst, n_lead, n_cut, n_cap), after = _stepped(sim, STEPS)
    print('queue, %s mode: worst |GPU - oracle| %.2e, %d agent-steps with a leader, %d cut by the rule, %d windows capped' % (mode, worst, n_lead, n_cut, n_cap))
    assert n_lead > 200 and n_cut > 0 and (n_cap > 0 or mode == 'cut')
    assert (after['leader'].reshape(2, 4)[:, 1:] == np.array([[0, 1, 2], [4, 5, 6]])).all() and (after['leader'][[0, 4]] == -1).all()


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_platoon_with_retirement_and_departure(ctx, stock, mode):
    """G2b.  Four cars 8.3 m apart near the end of one route, retirement and departure on, no signals, 45 steps: the first car arrives and
    leaves the scene, and the car behind it has no leader from the next step on.  Every driving agent of every step equals the oracle step."""
    sim = _queue(ctx, stock, mode, signals=False, start=np.array([[600, 500, 400, 300], [610, 505, 400, 295]]))
    (worst, n_lead, n_cut, n_cap), after = _stepped(sim, 45)
    print('platoon, %s mode: worst |GPU - oracle| %.2e, %d with a leader, %d cut by the rule, %d capped, done %s' % (mode, worst, n_lead, n_cut, n_cap, after['done']))
    assert n_lead > 100 and after['done'][[0, 4]].all() and after['absent'][[0, 4]].all() and (after['leader'][[1, 5]] == -1).all()


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_with_a_scripted_actor(ctx, stock, mode):
    """G2c.  Four agents and ONE scripted car per instance (the pool is [4 agents | 1 actor]; instance 0 has the stock car that drives straight
    on from the west), the agents on the route from the west behind it.  Every driving agent of every step equals the oracle step with the
    actor's row, as the device wrote it, among the others; an agent is led by the actor's row."""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_specs
    routes, dl, cd = stock
    west = [k for k, r in enumerate(routes) if abs(r[0, 1] + 3.0) < 0.5 and r[0, 0] < -25 and abs(r[-1, 1] + 3.0) < 0.5]
    assert west, 'no straight stock route from the west'
    sim = GR._batch(ctx, stock, np.full((2, 4), west[0]), np.array([[400, 300, 200, 100], [410, 305, 200, 100]]), mode,
                    traffic=scripted_traffic_specs(2, 1, 0, cd.distance_back_to_front_wheel, dt=0.2))
    sim.follow(**WIDE)
    assert sim.actor_row.cpu().numpy().tolist() == [4, 9] and int(sim.obs6.shape[0]) == 10
    led = 0
    tot = np.zeros(4)
    for s in range(STEPS):
        before = _snap(sim)
        sim.run(1)
        after = _snap(sim)
        w = _replay_step(sim, before, after, GS._pool_before(sim, before, after), before['absent'])
        tot = np.array([max(tot[0], w[0]), tot[1] + w[1], tot[2] + w[2], tot[3] + w[3]])
        led += int(np.isin(after['leader'], [4, 9]).sum())
    print('with an actor, %s mode: worst |GPU - oracle| %.2e, %d with a leader, %d led by the actor' % (mode, tot[0], tot[1], led))
    assert tot[1] > 100 and led > 0


# ---------------------------------------------------------------- G3: graph replay
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_graph_replay_in_chunks(ctx, stock, mode):
    """G3.  The queue under signals (and advice in speed mode) with following as 8 chunks of run(5, graph=True) on a side stream equals
    40 x run(1) plain, byte for byte, leader, gap and follow_cap included"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _queue(ctx, stock, mode, advise=mode == 'speed')
    for _ in range(STEPS):
        plain.run(1)
    a = _snap(plain)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _queue(side, stock, mode, advise=mode == 'speed')
        torch.cuda.synchronize()
        for _ in range(STEPS // 5):
            graph.run(5, graph=True)
        TS._same(a, _snap(graph), 'graph', skip=())
        assert 'leader' in a and (a['leader'] >= 0).sum() == 6
    finally:
        side.close()


# ---------------------------------------------------------------- G4: off
def _run_raw(sim, following, n, graph=0, desc=None):
    """the widest entry point with the structs of `sim` and `following` set on the context by hand"""
    sim._claim_context()
    sim.ctx.set_following(following)
    if sim._desc is None:
        sim._desc = sim._descriptor()
    try:
        sim.ctx.closed_loop_run(sim.ip, sim._desc if desc is None else desc, n, bool(graph), **sim._stage_structs())
    finally:
        sim.ctx.set_following(None)


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_off_means_off(ctx, stock, mode):
    """G4.  mpcx_set_following(NULL), an all-zero struct and stop_following() each give the bytes of a batch that never had following: 40
    steps of the queue, in which the batch with following does differ.  host staging (step_staged) with following equals run(1)."""
    from mpc_for_av_at_intersection_amd import _lib
    base = _queue(ctx, stock, mode, follow=None)
    base.run(STEPS)
    want = _snap(base)
    runs = {}
    sim = _queue(ctx, stock, mode, follow=None); _run_raw(sim, None, STEPS); runs['NULL'] = sim
    sim = _queue(ctx, stock, mode, follow=None); _run_raw(sim, _lib.FollowingC(), STEPS); runs['zero struct'] = sim
    sim = _queue(ctx, stock, mode); sim.stop_following(); sim.run(STEPS); runs['stop_following'] = sim
    for name, sim in runs.items():
        got = _snap(sim)
        assert 'leader' not in got
        TS._same(got, want, name, skip=())
    assert (runs['stop_following'].leader == -1).all()          # never written
    on = _queue(ctx, stock, mode); on.run(STEPS)
    got = _snap(on)
    assert (got['leader'] >= 0).any() and got['state'].tobytes() != want['state'].tobytes()
    X, Y = (_queue(ctx, stock, mode, retire=False) for _ in range(2))
    for s in range(10):
        X.run(1); Y.step_staged()
        TS._same(_snap(X), _snap(Y), s, skip=())
    assert (X.leader >= 0).any()


# ---------------------------------------------------------------- G5: the refusals
def test_refusals(ctx, stock):
    """G5.  MPCX_E_INVALID with a "following: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: leader, gap or cap NULL; n_rows != P; standstill, brake, lateral or heading not finite or not positive; time_gap
    negative or not finite; v_min not positive; reach outside 1..MPCX_MAX_REMAINING; a nonzero reserved word; the agent-sharded layout.  The
    stage calls refuse the same way.  In Python: follow() with malformed values."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _queue(ctx, stock, 'speed', retire=False)
    before = _snap(sim)
    fl = sim._following
    names = [n for n, _ in _lib.FollowingC._fields_]
    good = {n: getattr(fl, n) for n in names}
    make = lambda **kw: _lib.FollowingC(**dict(good, **kw))
    cut = sim.inter['cut_len']

    def refused(match, following, staged=True, **kw):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _run_raw(sim, following, n, graph, **kw)
        if staged:
            with pytest.raises(MpcxError, match=match):
                ctx.follow_step(sim.dl, _lib.STOP_SPEED, sim.state, sim.path, sim.path_off, sim.path_len, sim.traj_idx, cut, sim.obs6, sim.obs_off,
                                sim.obs_cnt, following, obs_skip=sim.obs_skip)
            with pytest.raises(MpcxError, match=match):
                ctx.follow_cap_step(following, sim.pre['xref'])
    for name in ('leader', 'gap', 'cap'):
        refused(r'mpcx error -1: following: %s is null' % name, make(**{name: None}))
    for n in (0, 7, 9, -8):
        refused(r'mpcx error -1: following: n_rows = %d is not P = 8' % n, make(n_rows=n))
    for name in ('standstill', 'brake', 'lateral', 'heading', 'v_min'):
        for v in (0.0, -1.0, float('inf'), float('nan')):
            refused(r'mpcx error -1: following: %s = .* must be finite and positive' % name, make(**{name: v}))
    for v in (-0.5, float('inf'), float('nan')):
        refused(r'mpcx error -1: following: time_gap = .* must be finite and not negative', make(time_gap=v))
    for r in (0, -3, _lib.MAX_REMAINING + 1):
        refused(r'mpcx error -1: following: reach = %d outside 1\.\.%d' % (r, _lib.MAX_REMAINING), make(reach=r))
    refused(r'mpcx error -1: following: the reserved word is not 0', make(reserved=1))
    _run_raw(sim, make(time_gap=0.0, reach=1), 0); _run_raw(sim, make(reach=_lib.MAX_REMAINING), 0)     # the limits themselves are accepted
    plain = _queue(ctx, stock, 'cut', signals=False, retire=False)
    plain_before = _snap(plain)
    desc = plain._descriptor()
    desc.exchange = _lib.SHARD_AGENTS
    for graph in (0, 1):
        for n in (0, 1):
            with pytest.raises(MpcxError, match='mpcx error -1: following: not supported in the agent-sharded layout'):
                _run_raw(plain, plain._following, n, graph, desc=desc)
    with pytest.raises(MpcxError, match='follow_step_batch: unknown stop mode 2'):
        ctx.follow_step(sim.dl, 2, sim.state, sim.path, sim.path_off, sim.path_len, sim.traj_idx, cut, sim.obs6, sim.obs_off, sim.obs_cnt, fl)
    ctx.synchronize()
    TS._same(_snap(sim), before, 'refused', skip=())
    TS._same(_snap(plain), plain_before, 'refused in the sharded layout', skip=())
    assert sim.steps_done == 0 and (sim.leader == -1).all() and not sim.follow_cap.any()
    for kw in (dict(standstill=0.0), dict(time_gap=-1.0), dict(brake=float('nan')), dict(v_min=0.0), dict(lateral=-1.0), dict(heading=float('inf')),
               dict(reach=0), dict(reach=_lib.MAX_REMAINING + 1)):
        with pytest.raises(ValueError):
            sim.follow(**kw)
    assert sim._following is fl
    sim.stop_following()
    assert sim._following is None and 'leader' not in sim.snapshot() and 'held' in sim.snapshot()


# ---------------------------------------------------------------- G6: a changed struct
def test_changed_struct_under_graph_replay():
    """G6.  The cached graph's key covers the struct by value: 10 steps replayed with the defaults, then standstill and time gap changed in
    place (the same buffers, the same descriptor) and 30 more replayed, equal the same sequence run plain, byte for byte -- and differ from
    40 steps under the defaults."""
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        stock = stock_routes(side)
        sims = [_queue(side, stock, 'cut', follow={}) for _ in range(3)]
        torch.cuda.synchronize()
        for sim, graph, change in zip(sims, (True, False, True), (True, True, False)):
            sim.run(10, graph=graph)
            if change:
                sim._following.standstill, sim._following.time_gap = 13.0, 2.0
            for _ in range(6):
                sim.run(5, graph=graph)
        a, b, c = (_snap(sim) for sim in sims)
        TS._same(a, b, 'changed struct', skip=())
        assert a['state'].tobytes() != c['state'].tobytes() and a['cut_len'].tobytes() != c['cut_len'].tobytes()
    finally:
        side.close()
