"""GPU tests of RIGHT OF WAY in the device-resident closed loop (mpcx_closed_loop_run_precedence, IntersectionBatch.give_way): an agent sees
the present cars whose precedence word is larger than its own as standing cars at their present pose.  The defining property: every driving
agent of every step equals the oracle step over its present rows with the yielding ones replaced by (x, y, 0, yaw, 0, 0) -- on the scenes
whose outcomes tests/test_precedence_cpu.py pins on the CPU oracle alone (four straight routes: arrivals 56 / 66 / 78 / 93 in cut mode,
59 / 70 / 80 / 95 in speed mode; nobody within 600 steps when everybody yields).  Then: equal words are the scene run, off means off,
first come first served (MPCX_PRECEDENCE_ENTRY) against a fixed-order twin whose words the host build of the stamp rewrites, graph replay,
host staging, the refusals.  B = 2, T = 13, v0 = 0 throughout."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import torch

from tests import admit_helpers as AH
from tests import precedence_helpers as PH
from tests import scene_helpers as SH
from tests import speedref_helpers as S
from tests import test_gpu_respawn as GR
from tests import test_gpu_route as TR
from tests import test_gpu_scene as GS

pytestmark = pytest.mark.gpu

T = GR.T
KEYS = GS.KEYS
# arrival steps of the straight scene on the CPU oracle alone (precedence_helpers.scene_loop): precedence = agent index (the cut-mode figures
# are tests/test_precedence_cpu.py's) and the reversed order (loop.prec = [3, 2, 1, 0])
STRAIGHT = {'cut': [56, 66, 78, 93], 'speed': [59, 70, 80, 95]}
REVERSED = {'cut': [92, 58, 86, 56], 'speed': [80, 60, 79, 59]}


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
def stock13(ctx):
    """the routes of the eight-agent scene: (arm, 1) and (arm, 3) of every arm"""
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    return stock_routes(ctx, pairs=tuple(PH.scene('eight')[0]))


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp('precedence_ref')
    return types.SimpleNamespace(admit=AH.build_ref(d), stamp=PH.build_ref(d))


def _straight(c, stock, mode='cut', order=((0, 1, 2, 3), (3, 2, 1, 0))):
    """B = 2 instances of the four straight routes from index 0; order: the precedence words per instance, None = no precedence"""
    sim = GR._batch(c, stock, np.tile(np.array([1, 3, 5, 7]), (2, 1)), np.zeros((2, 4), dtype=np.int64), mode)
    if order is not None:
        sim.give_way(order=np.array(order))
    return sim


def _replay_step(sim, before, after, pool, absent, prec):
    """test_gpu_scene._replay_step with right of way: every DRIVING agent of the step replayed on the oracle with the obstacle list = its
    pool window minus its own row minus the absent rows, the rows whose word is larger than its own row's STANDING (precedence_helpers.view).
    hit_idx, cut_len, traj_idx, target_ind, status, done and absent identical, u and x within 2e-7 (that test's bar); a retired agent's
    buffers are unchanged.  Returns (worst difference, number of agents for which the standing view and the plain view give different conflicts)."""
    from oracle import oracle_py as orc
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    speed = sim.stop_mode == 'speed'
    stop = sim.stop_index() if speed else None
    worst, differs = 0.0, 0
    for p in range(sim.P):
        if before['done'][p]:
            for k in KEYS:
                if k != 'applied':
                    assert before[k][p].tobytes() == after[k][p].tobytes(), (p, k)
            assert not after['applied'][p].any()
            continue
        present = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p] and not absent[r]]
        args = (po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p])
        rest = (int(before['traj_idx'][p]), int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                sim.ip.cutoff_margin)
        step = (lambda rows: S.agent_step(*args, rows, *rest, v_ref=sim.v_ref)) if speed else (lambda rows: orc.agent_step(*args, rows, *rest))
        r = step(PH.view(pool, present, prec[o_skip[p]], prec))
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        if speed:
            got = (after['traj_idx'][p], stop[p], after['target_ind'][p], after['hit_idx'][p], after['status'][p])
            assert (r['traj_idx'], r['stop'], r['target_ind'], want_hit, r['sol'].status) == got, (p, got)
            assert after['cut_len'][p] == (r['stop'] if r['hit'] is not None else ln[p]), p
        else:
            got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p])
            assert (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status) == got, (p, r['traj_idx'], r['cut'], want_hit, got)
        assert r['sol'].status == 0
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        # retirement and departure as the step's last launch leaves them: mpc.is_goal on the state after the plant step
        arrived = SH.is_goal(after['state'][p], tab[off[p] + ln[p] - 1], after['target_ind'][p], ln[p] if speed else after['cut_len'][p])
        assert bool(after['done'][p]) == arrived and after['absent'][o_skip[p]] == int(arrived), (p, arrived)
        if any(prec[q] > prec[o_skip[p]] for q in present):
            r2 = step(PH.view(pool, present, prec[o_skip[p]], prec, mode='all'))
            differs += (r2['hit'] is None) != (r['hit'] is None)
    assert worst < 2e-7, worst
    return worst, differs


def _stepped(sim, steps, until_done=False):
    """run(1) + snapshot() with the oracle replay of every step; returns (per-step `after` snapshots, worst, differs)"""
    recs, worst, differs = [], 0.0, 0
    for s in range(steps):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        assert np.array_equal(before['precedence'], after['precedence']) or sim._precedence.mode == 2
        w, d = _replay_step(sim, before, after, GS._pool_before(sim, before, after), before['absent'], before['precedence'])
        worst, differs = max(worst, w), differs + d
        recs.append(after)
        if until_done and after['done'].all():
            break
    return recs, worst, differs


def _arrivals(recs, P):
    out = np.full(P, -1)
    for s, r in enumerate(recs):
        out[(out < 0) & (r['done'] != 0)] = s + 1
    return out.tolist()


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_straight_routes_on_the_oracle(ctx, stock, mode):
    """G1.  The four straight routes from index 0, FIXED precedence by agent index in instance 0 and reversed in instance 1, departure on,
    until everybody has arrived.  After every step every driving agent equals the oracle step over its present rows with the yielding ones
    standing.  Both instances arrive at the steps of the CPU oracle's run.  Not vacuous: there are steps in which the plain view would have
    given a different conflict."""
    sim = _straight(ctx, stock, mode)
    recs, worst, differs = _stepped(sim, 130, until_done=True)
    arr = _arrivals(recs, sim.P)
    print('%s: worst |GPU - oracle| %.2e over %d steps, arrivals %s, %d agent-steps where the rule changed the conflict' % (mode, worst, len(recs), arr, differs))
    assert arr[:4] == STRAIGHT[mode] and arr[4:] == REVERSED[mode] and differs > 20
    assert recs[-1]['absent'].all() and np.array_equal(recs[-1]['precedence'], [0, 1, 2, 3, 3, 2, 1, 0])


# ---------------------------------------------------------------- G2
def test_eight_agents_on_the_oracle(ctx, stock13):
    """G2a.  The eight-agent scene (agents 0-3 on (arm, 1) from index k = round(10 / dl), agents 4-7 on (arm, 3) from index 0, behind them
    on the same arm), precedence = agent index, first 60 steps: the same replay; agent 0 has arrived by step 48 as on the CPU."""
    pairs, start = PH.scene('eight')
    sim = GR._batch(ctx, stock13, np.tile(np.arange(8), (2, 1)), np.tile(np.array(start), (2, 1)))
    sim.give_way(order=np.tile(np.arange(8), (2, 1)))
    recs, worst, differs = _stepped(sim, 60)
    arr = _arrivals(recs, sim.P)
    print('eight agents: worst |GPU - oracle| %.2e, arrivals so far %s, %d changed conflicts' % (worst, arr, differs))
    assert arr[0] == arr[8] == 48 and sum(a > 0 for a in arr) == 2 and differs > 20


def test_scripted_traffic_keeps_its_zero_word(ctx, stock):
    """G2b.  test_gpu_scene's shared-exit pair with the stock pair of scripted cars ([2 agents | 2 actors]); agent words (1, 2), the actors'
    words zero: both agents see the scripted cars moving, agent 0 sees agent 1 standing.  The same replay over 55 steps, the actors' rows as
    the device wrote them; the scripted cars never notice."""
    sim, plain = GS._pair(ctx, stock, backs=(20.0,), traffic=True), GS._pair(ctx, stock, backs=(20.0,), traffic=True)
    sim.give_way(order=np.array([[1, 2]]))
    assert sim.snapshot()['precedence'].tolist() == [1, 2, 0, 0] and sim.actor_row.cpu().numpy().tolist() == [2, 3]
    recs, worst, _ = _stepped(sim, 55)
    print('with traffic: worst |GPU - oracle| %.2e, arrivals %s' % (worst, _arrivals(recs, 2)))
    assert _arrivals(recs, 2)[0] > 0
    plain.run(55)
    assert recs[-1]['traffic_state'].tobytes() == plain.snapshot()['traffic_state'].tobytes()


# ---------------------------------------------------------------- G3
def _same(a, b, what, skip=('precedence',)):
    assert sorted(k for k in a if k not in skip) == sorted(k for k in b if k not in skip), what
    for k in b:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_equal_words_are_the_scene_run(ctx, stock):
    """G3.  With all words equal nobody yields in the rule's sense: after every one of 40 steps every buffer equals the scene run's, bit for
    bit (the PREC instantiations against the SCENE ones)."""
    a, b = _straight(ctx, stock, order=((7,) * 4, (-3,) * 4)), _straight(ctx, stock, order=None)
    for s in range(40):
        a.run(1); b.run(1)
        _same(a.snapshot(), b.snapshot(), s)
    assert 'precedence' in a.snapshot() and 'precedence' not in b.snapshot()


def _entry(sim, precedence, n, graph=0, **over):
    """mpcx_closed_loop_run_precedence itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, retire=sim._retire, scene=sim._scene, admit=sim._admit, respawn=sim._respawn, routes=sim._routes)
    st.update(over)
    ref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_precedence(c._ctx, C.byref(cip), C.byref(st['desc']), None, ref(sim._opts), ref(st['retire']), ref(st['scene']),
                                                 ref(st['admit']), ref(st['respawn']), ref(st['routes']), ref(precedence), int(n), int(graph)))


def test_off_means_off(ctx, stock):
    """G4.  precedence = NULL and an all-zero struct through mpcx_closed_loop_run_precedence, and yield_to_everyone(), each give the bytes of
    mpcx_closed_loop_run_routes: 60 steps of the routed batch of tests/test_gpu_route.py (admission, respawn and routes on), path_off and
    path_len and the episode table included."""
    from mpc_for_av_at_intersection_amd import _lib
    base = TR._routed(ctx, stock)
    TR._entry(base, base._routes, 60)
    want = base.snapshot()
    runs = {}
    sim = TR._routed(ctx, stock); _entry(sim, None, 60); runs['NULL'] = sim
    sim = TR._routed(ctx, stock); _entry(sim, _lib.PrecedenceC(), 60); runs['zero struct'] = sim
    sim = TR._routed(ctx, stock); sim.give_way('entry'); sim.yield_to_everyone(); sim.run(60); runs['yield_to_everyone'] = sim
    for name, sim in runs.items():
        got = sim.snapshot()
        assert 'precedence' not in got
        _same(got, want, name, skip=())
        for k in ('ep_i32', 'ep_f64', 'path_off', 'path_len'):
            assert getattr(sim, k).cpu().numpy().tobytes() == getattr(base, k).cpu().numpy().tobytes(), (name, k)
    assert int(base.clock.item()) == 60


# ---------------------------------------------------------------- G5
def _entry_batch(c, stock, log=0):
    sim = TR._routed(c, stock, log=log)
    sim.give_way('entry')
    return sim


def test_entry_mode_equals_a_fixed_order_the_host_rewrites(ctx, libs, stock):
    """G5.  First come, first served on the routed batch of tests/test_gpu_route.py (two arms x two slots, G = 3, admission, respawn and
    routes; B = 2).  X runs MPCX_PRECEDENCE_ENTRY.  Y runs MPCX_PRECEDENCE_FIXED, and before every run(1) the host -- the host build of the
    admission rule to know who this step admits, then the host build of the stamp -- rewrites Y's words.  After every one of 150 steps prec
    of X equals the numpy restatement applied step by step, and every buffer of X equals Y's bit for bit; vehicles did respawn, and a
    respawned vehicle's word is larger than that of everybody who was in the scene when it entered."""
    X, Y = _entry_batch(ctx, stock), TR._routed(ctx, stock)
    Y.give_way(order=np.zeros((2, 4), dtype=np.int64))
    own, off, cnt = (t.cpu().numpy() for t in (Y.obs_skip, Y.obs_off, Y.obs_cnt))
    rows = int(Y.obs6.shape[0])
    want = np.zeros(rows, np.int32)
    later = 0
    for s in range(150):
        snap = Y.snapshot()
        gate = AH.Case(snap['state'], own=own, wait=snap['wait'].copy(), done=snap['done'].copy(), absent=snap['absent'].copy(), gap=1.0,
                       radius=Y.ip.radius, centers=Y.ip.circle_centers, obs_off=off, obs_cnt=cnt, clock=int(Y.clock.item()),
                       entered=snap['entered_step'].copy())
        AH.host_step(libs.admit, gate)
        words = snap['precedence'].copy()
        PH.host_stamp(libs.stamp, words, gate.entered, own, off, rows)
        PH.stamp_numpy(want, gate.entered, own, off, rows)
        for q in np.flatnonzero((snap['entered_step'] < 0) & (gate.entered >= 0)):          # admitted in this step
            there = [r for r in range(off[q], off[q] + cnt[q]) if r != own[q] and not snap['absent'][r]]      # in the scene before this step
            assert all(words[r] < words[own[q]] for r in there), (s, q)
            later += len(there) > 0 and s > 0
        Y.prec.copy_(torch.from_numpy(words).to(Y.prec.device))
        X.run(1); Y.run(1)
        x, y = X.snapshot(), Y.snapshot()
        assert np.array_equal(x['precedence'], want) and np.array_equal(y['precedence'], want), s
        _same(x, y, s, skip=())
        for k in ('ep_i32', 'ep_f64', 'path_off', 'path_len'):
            assert getattr(X, k).cpu().numpy().tobytes() == getattr(Y, k).cpu().numpy().tobytes(), (s, k)
    ep = X.episodes()
    print('entry mode: %d episodes in 150 steps, %d entries behind somebody; words %s' % (len(ep), later, want.tolist()))
    assert len(ep) >= 4 and (ep['generation'] > 0).any() and later >= 2 and int(X.clock.item()) == 150


# ---------------------------------------------------------------- G6
def test_graph_replay_in_chunks(ctx, stock):
    """G6.  G5's batch as 15 chunks of run(7, graph=True) on a side stream equals 105 x run(1) plain, byte for byte: the final snapshot
    (the words included), the episode table and path_off / path_len -- the stamp reads device words only, so the one captured step keeps
    stamping as vehicles enter."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _entry_batch(ctx, stock)
    for _ in range(105):
        plain.run(1)
    a = plain.snapshot()
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _entry_batch(side, stock)
        torch.cuda.synchronize()
        for _ in range(15):
            graph.run(7, graph=True)
        b = graph.snapshot()
        _same(a, b, 'graph', skip=())
        assert int(graph.clock.item()) == 105 and len(np.unique(a['precedence'])) > 4 and len(plain.episodes()) >= 2
        for k in ('ep_i32', 'ep_f64', 'path_off', 'path_len'):
            assert getattr(plain, k).cpu().numpy().tobytes() == getattr(graph, k).cpu().numpy().tobytes(), k
    finally:
        side.close()


# ---------------------------------------------------------------- G7
def test_host_staging_equals_the_loop(ctx, stock):
    """G7.  The head of a step staged from the host: Context.admit_step(precedence=<ENTRY struct>) -- admission, then the stamp -- followed
    by run(1) of a batch WITHOUT admission whose precedence is FIXED equals run(1) of the batch with admission and MPCX_PRECEDENCE_ENTRY in
    the loop: every buffer, wait, entered_step, the clock and the words, after every one of 50 steps of the straight scene entered on a
    schedule."""
    from mpc_for_av_at_intersection_amd import _lib
    wait = np.array([[0, 3, 0, 5], [6, 0, 2, 0]])
    X, Y = _straight(ctx, stock, order=None), _straight(ctx, stock, order=None)
    for sim in (X, Y):
        sim.enter_on_schedule(wait, gap=1.0)
        sim.give_way('entry')
    admit, entry = Y._admit, Y._precedence
    Y._admit = None
    Y._precedence = _lib.PrecedenceC(Y.prec.data_ptr(), Y.stand.data_ptr(), int(Y.prec.shape[0]), _lib.PRECEDENCE_FIXED)
    Y._desc = None
    for s in range(50):
        X.run(1)
        ctx.admit_step(Y.ip, Y.state, Y.obs_off, Y.obs_cnt, Y.obs_skip, Y.done, Y.absent, admit, precedence=entry)
        Y.run(1)
        x, y = X.snapshot(), Y.snapshot()
        _same(x, y, s, skip=('wait', 'entered_step'))
        for k in ('wait', 'entered_step', 'clock'):
            assert getattr(X, k).cpu().numpy().tobytes() == getattr(Y, k).cpu().numpy().tobytes(), (s, k)
    e = X.entered_step.cpu().numpy()
    assert (e >= wait.reshape(-1)).all() and np.array_equal(x['precedence'], e * 64 + np.tile(np.arange(4), 2)), (e, x['precedence'])


# ---------------------------------------------------------------- G8
def test_refusals(ctx, stock):
    """G8.  MPCX_E_INVALID with a "precedence: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: an unknown mode, precedence without a scene, prec or stand missing, n_rows that is not the pool's row count,
    MPCX_PRECEDENCE_ENTRY without admission.  The scene's own refusals are inherited: the agent-sharded layout, more than one linearisation
    pass, step_staged().  In Python: give_way() without a scene, order='entry' without admission, a bad order array, a run beyond the last
    step whose word fits; keep_driving(), retire_at_goal() and -- for order='entry' -- enter_now() drop precedence, yield_to_everyone()
    switches it off alone."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _straight(ctx, stock)
    before = sim.snapshot()
    pc = sim._precedence
    good = dict(prec=pc.prec, stand=pc.stand, n_rows=pc.n_rows, mode=pc.mode)
    make = lambda **kw: _lib.PrecedenceC(**dict(good, **kw))

    def refused(match, precedence, **over):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _entry(sim, precedence, n, graph, **over)
    for mode in (0, 3, -1):
        refused(r'mpcx error -1: precedence: unknown mode %d' % mode, make(mode=mode))
    refused(r'mpcx error -1: precedence: precedence needs a scene', pc, scene=None)
    refused(r'mpcx error -1: precedence: precedence needs a scene', pc, scene=_lib.SceneC())
    refused(r'mpcx error -1: precedence: .*prec is null', make(prec=None))
    refused(r'mpcx error -1: precedence: .*stand is null', make(stand=None))
    refused(r'mpcx error -1: precedence: n_rows = 7, the pool has 8 rows', make(n_rows=7))
    refused(r'mpcx error -1: precedence: n_rows = 9, the pool has 8 rows', make(n_rows=9))
    refused(r'mpcx error -1: precedence: MPCX_PRECEDENCE_ENTRY needs admission', make(mode=_lib.PRECEDENCE_ENTRY))
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 2, 4, sim.obs6.data_ptr()
    refused(r'mpcx error -1: scene: not supported in the agent-sharded layout', pc, desc=shard)
    ctx.set_linearisation_passes(2)
    try:
        sim.lin_passes = 2
        refused(r'mpcx error -1: retire', pc)
        with pytest.raises(MpcxError, match='lin_passes'):
            sim.run(1)
    finally:
        sim.lin_passes = 1
        ctx.set_linearisation_passes(1)
    with pytest.raises(MpcxError, match='step_staged'):
        sim.step_staged()
    # the stage-level call refuses the same way, before the admission stage is launched
    e = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=ctx.device)
    wait, entered, clock = e(torch.int32, sim.P), e(torch.int32, sim.P), e(torch.int32, 1)
    ad = _lib.AdmitC(wait.data_ptr(), entered.data_ptr(), clock.data_ptr(), 0, 1.0)
    for bad, match in ((make(mode=5), 'precedence: unknown mode 5'), (make(n_rows=3), 'precedence: n_rows = 3'), (make(stand=None), 'stand is null')):
        with pytest.raises(MpcxError, match=match):
            ctx.admit_step(sim.ip, sim.state, sim.obs_off, sim.obs_cnt, sim.obs_skip, sim.done, sim.absent, ad, precedence=bad)
    ctx.synchronize()
    assert int(clock.item()) == 0
    _same(sim.snapshot(), before, 'refused', skip=())
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # ---- Python
    for bad in ('exit', np.zeros((2, 3), dtype=np.int64), np.zeros((2, 4)), np.full((2, 4), 2 ** 40)):
        with pytest.raises(ValueError):
            sim.give_way(order=bad)
    with pytest.raises(MpcxError, match='needs admission'):
        sim.give_way('entry')
    assert sim._precedence is pc
    bare = GS._pair(ctx, stock, leave=False)
    with pytest.raises(MpcxError, match='needs a scene'):
        bare.give_way(order=np.zeros((2, 2), dtype=np.int64))
    assert bare._precedence is None and 'precedence' not in bare.snapshot()
    sim.yield_to_everyone()
    assert sim._precedence is None and sim._scene is not None and 'precedence' not in sim.snapshot()
    sim.enter_on_schedule(np.zeros((2, 4), dtype=np.int64), gap=1.0)
    sim.give_way('entry')
    assert sim._precedence.mode == _lib.PRECEDENCE_ENTRY
    sim.steps_done = _lib.PRECEDENCE_MAX_STEP
    with pytest.raises(MpcxError, match='fits int32'):
        sim.run(1)
    sim.steps_done = 0
    sim.enter_now()
    assert sim._precedence is None
    for off in ('keep_driving', 'retire_at_goal'):
        s2 = _straight(ctx, stock)
        getattr(s2, off)()
        assert s2._precedence is None and 'precedence' not in s2.snapshot()
    s3 = _straight(ctx, stock)
    s3.enter_on_schedule(np.zeros((2, 4), dtype=np.int64))
    s3.enter_now()
    assert s3._precedence is not None and s3._precedence.mode == _lib.PRECEDENCE_FIXED
