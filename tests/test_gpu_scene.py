"""GPU tests of DEPARTURE in the device-resident closed loop (mpcx_closed_loop_run_scene, IntersectionBatch.retire_at_goal(leave_scene=True)):
an arrived agent's pool row stops existing for everybody else.  Two agents that share an exit arm -- the second can only arrive once the
first has left the scene -- replayed step by step on the CPU oracle with the obstacle list "pool window minus own row minus absent rows",
with scripted traffic (the mask index goes through the row map), the run log, the speed stop mode, graph replay, both QP solvers, a preset
mask, and: off means off, the refusals, keep_driving().  The host build of the rules is tests/test_scene_cpu.py.

Arrival steps, established on the CPU oracle alone (tests/scene_helpers.OracleLoop, T = 13, v0 = 0, agent 0 on route (1, 2) 10 m before its
last point, agent 1 on route (2, 1) `back` m before its last point):
    cut mode,   back 20 m: (29, 50) with departure, (29, never within 150) without       back 25 m: (33, 52) / (33, never)
    speed mode, back 20 m: (25, 45) with departure, (25, 74) without (there the second car creeps up behind the parked one)
The stock pair of scripted cars changes none of the cut-mode numbers."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import scene_helpers as SH
from tests import speedref_helpers as S

pytestmark = pytest.mark.gpu

T = 13
STEPS = 70
KEYS = ('state', 'applied', 'traj_idx', 'target_ind', 'prev_cut', 'x', 'u', 'status', 'iters', 'kkt', 'hit_idx', 'hit_xy', 'cut_len', 'xref',
        'reaches_end', 'xbar')


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


def _ip(cd, dl):
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams
    return InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                             circle_centers=np.asarray(cd.circle_centers).ravel())


def _pair(c, stock, backs=(20.0, 25.0), leave=True, traffic=False, mode='cut', routes_ab=(1, 2), start_a=None):
    """len(backs) instances x 2 agents: agent 0 on route routes_ab[0] started 10 m before its last point (or at start_a), agent 1 on route
    routes_ab[1] started backs[b] m before its last point; traffic: the stock pair of scripted cars in every instance.
    leave: True = retire_at_goal(leave_scene=True), False = retire_at_goal(), None = no retirement"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch, scripted_traffic_specs
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    routes, dl, cd = stock
    B = len(backs)
    ra, rb = routes_ab
    route = np.tile(np.array([ra, rb]), (B, 1))
    start = np.zeros((B, 2), dtype=np.int64)
    start[:, 0] = len(routes[ra]) - 1 - int(round(10.0 / dl)) if start_a is None else start_a
    start[:, 1] = [len(routes[rb]) - 1 - int(round(b / dl)) for b in backs]
    kw = {}
    params = MpcParams(T=T, L=cd.distance_back_to_front_wheel)
    if mode == 'speed':
        import mpc_for_av_at_intersection_amd.lib.mpc_with_speed as ws
        params = dataclasses.replace(ws.params(cd, 0.2), L=cd.distance_back_to_front_wheel)
        kw['stop_mode'] = 'speed'
    if traffic:
        assert B == 1
        kw['traffic'] = scripted_traffic_specs(1, 2, 0, cd.distance_back_to_front_wheel, dt=params.dt)       # instance 0: the stock pair
    sim = IntersectionBatch(c, params, _ip(cd, dl), routes, dl, route, start, **kw)
    if leave is not None:
        sim.retire_at_goal(leave_scene=leave)
    return sim


def _pool_before(sim, before, after):
    """the pool as the step before -> after saw it: the agents' rows packed from the state and the applied controls before the step, the
    scripted cars' rows as the device wrote them (the pool is filled at the start of a step and not touched again)"""
    packed = np.column_stack([before['state'], before['applied'][:, 1], before['applied'][:, 0]])
    if sim.traffic is None:
        return packed
    pool = after['obs6']
    assert np.array_equal(pool[sim.ego_row.cpu().numpy()], packed)
    return pool


def _replay_step(sim, before, after, pool, absent, include=()):
    """Every DRIVING agent of the step replayed on the oracle with the obstacle list = its pool window minus its own row minus the absent
    rows (relative order kept); every retired agent's buffers are unchanged.  Integer decisions and status identical, u and x within 2e-7
    (helpers.replay_all_on_oracle's bar).  Returns (worst difference, {agent: oracle hit index with the rows `include` put back})."""
    from oracle import oracle_py as orc
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    speed = sim.stop_mode == 'speed'
    stop = sim.stop_index() if speed else None
    worst, other = 0.0, {}
    for p in range(sim.P):
        if before.get('done') is not None and before['done'][p]:
            for k in KEYS:
                if k != 'applied':
                    assert before[k][p].tobytes() == after[k][p].tobytes(), (p, k)
            assert not after['applied'][p].any()
            continue
        window = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p]]
        present = [r for r in window if not absent[r]]
        args = (po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p])
        rest = (int(before['traj_idx'][p]), int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                sim.ip.cutoff_margin)
        step = (lambda rows: S.agent_step(*args, pool[rows], *rest, v_ref=sim.v_ref)) if speed else (lambda rows: orc.agent_step(*args, pool[rows], *rest))
        r = step(present)
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        if speed:
            assert (r['traj_idx'], r['stop'], r['target_ind'], want_hit, r['sol'].status) == \
                (after['traj_idx'][p], stop[p], after['target_ind'][p], after['hit_idx'][p], after['status'][p]), p
            assert after['cut_len'][p] == (r['stop'] if r['hit'] is not None else ln[p]), p
        else:
            assert (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status) == \
                (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p]), \
                (p, r['traj_idx'], r['cut'], r['target_ind'], want_hit, after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p])
        assert r['sol'].status == 0
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        if include:
            r2 = step(sorted(set(present) | (set(include) & set(window))))
            other[p] = -1 if r2['hit'] is None else int(r2['hit'][2])
    assert worst < 2e-7, worst
    return worst, other


def _stepped(sim, steps, twin=None, include=()):
    """run(1) + snapshot() `steps` times with the oracle replay of every step; returns the per-step records"""
    recs = []
    worst = 0.0
    for s in range(steps):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        absent = before['absent'] if 'absent' in before else np.zeros(int(sim.obs6.shape[0]), np.int32)
        pool = _pool_before(sim, before, after)
        w, other = _replay_step(sim, before, after, pool, absent, include)
        worst = max(worst, w)
        rec = dict(before=before, after=after, pool=pool, absent=absent.copy(), other=other)
        if twin is not None:
            twin.run(1)
            rec['twin'] = twin.snapshot()
        recs.append(rec)
    return recs, worst


def _arrivals(recs, P):
    """1-based step in which done[q] was set, -1 = not yet"""
    out = np.full(P, -1)
    for s, r in enumerate(recs):
        out[(out < 0) & (r['after']['done'] != 0)] = s + 1
    return out.tolist()


@pytest.fixture(scope='module')
def shared(ctx, stock):
    """test 1's batch (B = 2, A = 2, leave_scene=True, a log attached) stepped 70 times beside its retire-only twin"""
    sim, twin = _pair(ctx, stock), _pair(ctx, stock, leave=False)
    log = sim.attach_log(STEPS + 10)
    recs, worst = _stepped(sim, STEPS, twin=twin)
    return dict(sim=sim, twin=twin, log=log, recs=recs, worst=worst)


def test_shared_exit(ctx, stock, shared):
    """Test 1.  B = 2, A = 2: agent 0 on route (1, 2) 10 m before its last point, agent 1 on route (2, 1) 20 m (instance 0) / 25 m
    (instance 1) before its last point, leave_scene=True, 70 steps of run(1) + snapshot().  Every driving agent of every step equals the
    oracle step with the obstacle list minus the absent rows; arrivals at steps (29, 50) and (33, 52); absent is set for exactly the arrived
    agents' own rows from the step of their arrival on; agent 1 has a conflict in exactly the steps before agent 0's departure;
    run_until_done(150, chunk=8) ends early with nobody driving.  The retire-only twin is bit-identical until the first arrival of each
    instance, and in it agent 1 has not arrived after 150 steps: the gap this closes."""
    sim, twin, recs = shared['sim'], shared['twin'], shared['recs']
    print('shared exit: worst |GPU - oracle| %.2e over %d steps' % (shared['worst'], len(recs)))
    arr = _arrivals(recs, sim.P)
    assert arr == [29, 50, 33, 52], arr
    own = sim.obs_skip.cpu().numpy()
    assert own.tolist() == [0, 1, 2, 3] and sim.absent.shape == (4,)
    for s, r in enumerate(recs):
        want = np.zeros(4, np.int32)
        want[own[[q for q in range(4) if 0 < arr[q] <= s + 1]]] = 1
        assert np.array_equal(r['after']['absent'], want), (s, r['after']['absent'])
        assert np.array_equal(r['after']['absent'], (r['after']['done'] != 0).astype(np.int32))
        for b, (lead, follow) in enumerate(((0, 1), (2, 3))):
            if s < arr[follow]:         # the follower drives: a conflict exactly while the leader is in the scene
                assert (r['after']['hit_idx'][follow] >= 0) == (s < arr[lead]), (s, b, r['after']['hit_idx'])
            if s + 1 < arr[lead]:       # before the first arrival of the instance the retire-only twin is the same run
                for k in KEYS + ('done', 'steps_driven'):
                    assert r['after'][k][2 * b:2 * b + 2].tobytes() == r['twin'][k][2 * b:2 * b + 2].tobytes(), (s, b, k)
    assert np.array_equal(recs[-1]['after']['steps_driven'], arr)
    twin.run(150 - STEPS)
    t = twin.snapshot()
    assert t['done'].tolist() == [1, 0, 1, 0] and t['steps_driven'].tolist() == [29, 150, 33, 150], (t['done'], t['steps_driven'])
    assert (t['hit_idx'][[1, 3]] >= 0).all()
    fresh = _pair(ctx, stock)
    taken = fresh.run_until_done(150, chunk=8)
    assert taken == 56 < 150 and fresh.active_count() == 0, taken
    assert fresh.steps_driven.cpu().numpy().tolist() == arr
    fresh.check()


def test_with_scripted_traffic(ctx, stock):
    """Test 2.  Instance 0 of test 1 plus the stock pair of scripted cars: the pool is [2 agents | 2 actors], the agents' own rows come
    from the row map.  Same oracle replay, the actors' rows (as the device wrote them) appended to the obstacle list; arrivals (29, 50); the
    scripted cars never notice: traffic_state equals a retire-only batch's after the same steps, bit for bit."""
    sim, plain = _pair(ctx, stock, backs=(20.0,), traffic=True), _pair(ctx, stock, backs=(20.0,), traffic=True, leave=False)
    assert sim.obs_skip.cpu().numpy().tolist() == sim.ego_row.cpu().numpy().tolist() == [0, 1] and sim.actor_row.cpu().numpy().tolist() == [2, 3]
    assert sim.absent.shape == (4,)
    recs, worst = _stepped(sim, 55)
    print('with traffic: worst |GPU - oracle| %.2e' % worst)
    assert _arrivals(recs, 2) == [29, 50]
    assert recs[-1]['after']['absent'].tolist() == [1, 1, 0, 0]
    assert [r['after']['hit_idx'][1] >= 0 for r in recs[:50]] == [s < 29 for s in range(50)]
    plain.run(55)
    assert recs[-1]['after']['traffic_state'].tobytes() == plain.snapshot()['traffic_state'].tobytes()
    assert np.abs(recs[-1]['after']['obs6'][2:, 2]).max() > 1.0        # the cars have started


def test_run_log(shared):
    """Test 3.  The log attached to test 1's batch: every logged clearance of a driving agent is the numpy restatement over the present rows
    of its window within 1e-12 (+inf once the other has left); the followers' contact_step is "none" and their min_clearance >= 0 although
    they end on top of where the leaders stand; goal_step == steps_driven == the arrival steps."""
    sim, log, recs = shared['sim'], shared['log'], shared['recs']
    rows, out = log.rows(), log.outcomes()
    arr = _arrivals(recs, sim.P)
    centers, radius = np.asarray(sim.ip.circle_centers).reshape(2, 2), sim.ip.radius
    assert rows.shape == (max(arr), sim.P)
    checked = 0
    for s, r in enumerate(recs):
        for p in range(sim.P):
            if s >= arr[p]:
                continue
            b = p // 2
            present = [q for q in (2 * b, 2 * b + 1) if q != p and not r['absent'][q]]
            want = SH.clearance(r['pool'], p, present, centers, radius)
            got = rows['clearance'][s, p]
            assert (got == want) if np.isinf(want) else abs(got - want) <= 1e-12, (s, p, got, want)
            assert np.isinf(want) == (s >= arr[p ^ 1]), (s, p)
            checked += 1
    assert checked == sum(arr)
    assert out['goal_step'].tolist() == arr == out['steps'].tolist() == recs[-1]['after']['steps_driven'].tolist()
    assert (out['contact_step'] == -1).all() and (out['min_clearance'] >= 0.0).all(), out
    end = recs[-1]['after']['state']
    assert np.hypot(*(end[1, :2] - end[0, :2])) < 2 * radius + 2.0          # ... where a parked leader would have been a contact


def test_speed_stop_mode(ctx, stock):
    """Test 4.  Instance 0 of test 1 with stop_mode='speed' and lib.mpc_with_speed.params(): the same replay with
    tests/speedref_helpers.agent_step.  Arrivals (25, 45), established on the CPU with that helper (the header has the numbers; without
    departure the second car arrives at step 74)."""
    sim = _pair(ctx, stock, backs=(20.0,), mode='speed')
    recs, worst = _stepped(sim, 50)
    print('speed mode: worst |GPU - oracle| %.2e' % worst)
    assert _arrivals(recs, 2) == [25, 45]
    assert recs[-1]['after']['absent'].tolist() == [1, 1]
    assert [r['after']['hit_idx'][1] >= 0 for r in recs[:45]] == [s < 25 for s in range(45)]


def _final(sim, log):
    snap = sim.snapshot()
    return snap, log.rows(), log.outcomes()


def test_graph_replay(ctx, stock):
    """Test 5a.  run(70, graph=True) on a side stream == run(70): every snapshot buffer, absent, the log's rows and outcomes, bit for bit
    -- done, absent and the queue length are device memory, so the one captured step departs agents as it is replayed."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _pair(ctx, stock)
    lp = plain.attach_log(STEPS)
    plain.run(STEPS)
    a = _final(plain, lp)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        g = _pair(side, stock)
        lg = g.attach_log(STEPS)
        torch.cuda.synchronize()
        g.run(STEPS // 3, graph=True)
        g.run(STEPS - STEPS // 3, graph=True)
        b = _final(g, lg)
    finally:
        side.close()
    assert a[0]['absent'].tolist() == [1, 1, 1, 1] and a[0]['steps_driven'].tolist() == [29, 50, 33, 52]
    for k in a[0]:
        assert a[0][k].tobytes() == b[0][k].tobytes(), k
    for name in a[1].dtype.names:
        assert a[1][name].tobytes() == b[1][name].tobytes(), name
    for k in a[2]:
        assert a[2][k].tobytes() == b[2][k].tobytes(), k


@pytest.mark.parametrize('solver', ['condensed', 'stage'])
def test_both_solvers(stock, solver):
    """Test 5b.  Test 1's replay with the QP solver forced (each draws its tickets up to the device-side queue length): parity with the
    oracle at every step and the same arrivals."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    try:
        c.set_qp_solver(solver)
        sim = _pair(c, stock)
        recs, worst = _stepped(sim, 55)
        print('%s: worst |GPU - oracle| %.2e' % (solver, worst))
        assert _arrivals(recs, 4) == [29, 50, 33, 52]
    finally:
        c.close()


def test_preset_mask(ctx, stock):
    """Test 6.  The stock ego (route (4, 1) from its first point) and a second agent on route (1, 2) 10 m before its last point, with the
    stock pair of scripted cars; the second car -- the one the stock scenario spawns on the ego's start pose -- is hidden from step 0 by
    presetting its word of the mask.  Every step equals the oracle step of a scene without that car.  Not vacuous, by the oracle alone:
    with the hidden row put back into the list the ego has a conflict in steps where it has none without (on the CPU oracle: steps 0-10).
    The second agent arrives at step 25 and departs in the same mask."""
    routes, dl, cd = stock
    sim = _pair(ctx, stock, backs=(10.0,), traffic=True, routes_ab=(6, 1), start_a=0)
    hidden = int(sim.actor_row[1])
    assert hidden == 3
    sim.absent[hidden] = 1
    recs, worst = _stepped(sim, 30, include=(hidden,))
    print('preset mask: worst |GPU - oracle| %.2e' % worst)
    differs = [s for s, r in enumerate(recs) if (r['other'][0] >= 0) != (r['after']['hit_idx'][0] >= 0)]
    print('steps in which the hidden car would have been a conflict of the ego:', differs)
    assert len(differs) >= 5 and differs[0] == 0
    assert _arrivals(recs, 2) == [-1, 25]
    assert recs[-1]['after']['absent'].tolist() == [0, 1, 0, 1]


def _same(a, b, what, keys=None):
    for k in (keys or a.keys()):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_off_means_off_and_refusals(ctx, stock):
    """Test 7.  leave_scene=False and scene=NULL / an all-zero struct are mpcx_closed_loop_run_retire: bit-identical runs across an
    arrival.  MPCX_E_INVALID ("scene: ...") before anything is launched, whatever n_steps is and with or without a graph: n_rows that is not
    the pool's row count, a scene without retirement, a null mask, an agent whose own row lies outside the pool, MPCX_SHARD_AGENTS; in
    Python leave_scene=True with exchange='rccl' -- the state is unchanged by all of them.  keep_driving() after a departure makes the car
    visible again: the follower's next step has a conflict."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import MpcParams, MpcxError
    routes, dl, cd = stock
    # ---- off means off
    ret, null, zero = (_pair(ctx, stock, backs=(20.0,), leave=False) for _ in range(3))
    ret.run(35)
    ctx.closed_loop_run(null.ip, null._descriptor(), 35, retire=null._retire, scene=None)
    ctx.closed_loop_run(zero.ip, zero._descriptor(), 35, retire=zero._retire, scene=_lib.SceneC())
    a = ret.snapshot()
    assert a['done'].tolist() == [1, 0] and 'absent' not in a and ret.absent is None
    _same(a, null.snapshot(), 'scene=NULL')
    _same(a, zero.snapshot(), 'all-zero scene')
    # ---- refusals
    sim = _pair(ctx, stock, backs=(20.0,))
    desc = sim._descriptor()
    before = sim.snapshot()

    def scene(**kw):
        c = _lib.SceneC()
        C.memmove(C.byref(c), C.byref(sim._scene), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def refused(match, d=desc, retire=sim._retire, sc=sim._scene):
        for graph in (False, True):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    ctx.closed_loop_run(sim.ip, d, n, graph, retire=retire, scene=sc)
    refused(r'mpcx error -1: scene: n_rows = 3', sc=scene(n_rows=3))
    refused(r'mpcx error -1: scene: n_rows = 5', sc=scene(n_rows=5))
    refused(r'mpcx error -1: scene: absent is null', sc=scene(absent=None))
    refused(r'mpcx error -1: scene: departure needs retirement', retire=None)
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 1, 2, sim.obs6.data_ptr()
    refused(r'mpcx error -1: scene: not supported in the agent-sharded layout', d=shard)
    bad_rows = torch.tensor([0, 2], dtype=torch.int32, device=sim.obs_skip.device)
    outside = sim._descriptor()
    outside.obs_skip = bad_rows.data_ptr()
    refused(r'mpcx error -1: scene: agent 1 sits in pool row 2 of 2', d=outside)
    none = sim._descriptor()
    none.obs_skip = None
    refused(r'mpcx error -1: scene: obs_skip is required', d=none)
    # retirement's own refusals stay as they are
    with pytest.raises(MpcxError, match=r'mpcx error -1: retire'):
        ctx.closed_loop_run(sim.ip, desc, 1, retire=_lib.RetireC(sim.done.data_ptr(), None, 1.5, 0.1), scene=sim._scene)
    with pytest.raises(MpcxError, match='step_staged'):
        sim.step_staged()
    sharded = IntersectionBatch(ctx, MpcParams(T=T, L=cd.distance_back_to_front_wheel), _ip(cd, dl), routes, dl, np.array([[1, 2]]),
                                np.array([[0, 0]]), agent_shard=(0, 1), exchange='rccl')
    with pytest.raises(MpcxError, match='leave_scene=True'):
        sharded.retire_at_goal(leave_scene=True)
    assert sharded.done is None and sharded._retire is None
    _same(before, sim.snapshot(), 'refused')
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # ---- keep_driving() brings a departed car back into view
    sim.run(32)
    s = sim.snapshot()
    assert s['done'].tolist() == [1, 0] and s['absent'].tolist() == [1, 0] and s['hit_idx'][1] == -1
    sim.keep_driving()
    sim.run(1)
    s = sim.snapshot()
    assert 'absent' not in s and 'done' not in s and s['hit_idx'][1] >= 0, s['hit_idx']
