"""GPU tests of retirement at the goal in the device-resident closed loop (mpcx_closed_loop_run_retire, IntersectionBatch.retire_at_goal):
a single ego among scripted cars is bit-identical to today's loop up to its arrival and frozen afterwards (cut and speed mode, both QP
solvers, graph replay), coupled agents see a retired one as a parked car, a batch in which everybody has arrived changes nothing, and the
refusals.  The host build of the rule is tests/test_retire_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_runlog_cpu import outcome_from_clearances

pytestmark = pytest.mark.gpu

# scripted_traffic_batch(B = 4, T = 13, A = 1, K = 2, seed = SEED): every ego arrives within [1, N - 10] steps in both stop modes (asserted
# below; instance 0 is the stock scenario, 82 steps at T = 13).  If a seed does not arrive, change the seed, never the assertion.
SEED, N = 0, 150
PER_AGENT = ('state', 'applied', 'traj_idx', 'target_ind', 'prev_cut', 'x', 'u', 'status', 'iters', 'kkt', 'hit_idx', 'hit_xy', 'cut_len', 'xref',
             'reaches_end', 'xbar')
FROZEN = tuple(k for k in PER_AGENT if k not in ('state', 'applied'))       # sol, pre, inter, target_ind, traj_idx (+ prev_len in speed mode)


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


def _single(c, stock, mode='cut', B=4):
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    routes, dl, cd = stock
    kw = {}
    if mode == 'speed':
        import mpc_for_av_at_intersection_amd.lib.mpc_with_speed as ws
        kw = dict(stop_mode='speed', mpc=ws.params(cd, 0.2))
    return scripted_traffic_batch(c, B=B, T=13, A=1, K=2, seed=SEED, routes=routes, dl=dl, cd=cd, **kw)


def _same(a, b, what, keys=None):
    for k in (keys or a.keys()):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _rows_same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for name in a.dtype.names:
        assert a[name].tobytes() == b[name].tobytes(), (what, name)


def _runs(c, stock, mode):
    """test 1's three batches: `plain` runs N steps with a log and no retirement, `snaps` are the per-step snapshots of an identical batch
    stepped with run(1), `ret` runs N steps with a log and retirement.  Host copies only (but for the retired batch itself)."""
    plain, twin, ret = (_single(c, stock, mode) for _ in range(3))
    lp = plain.attach_log(N)
    plain.run(N)
    snaps = []
    for _ in range(N):
        twin.run(1)
        snaps.append(twin.snapshot())
    lr = ret.attach_log(N)
    ret.retire_at_goal()
    c.closed_loop_stats(reset=True)
    ret.run(N)
    stats = c.closed_loop_stats(reset=True)
    return dict(plain_rows=lp.rows(), plain_out=lp.outcomes(), plain_final=plain.snapshot(), snaps=snaps, ret=ret, ret_log=lr, ret_rows=lr.rows(),
                ret_out=lr.outcomes(), ret_final=ret.snapshot(), stats=stats)


_CACHE = {}


@pytest.fixture(scope='module')
def runs(ctx, stock):
    def get(mode):
        if mode not in _CACHE:
            _CACHE[mode] = _runs(ctx, stock, mode)
        return _CACHE[mode]
    yield get
    _CACHE.clear()


def _assert_single_ego_parity(r, what):
    """the assertions of test 1 on a dict of _runs()"""
    goal = r['plain_out']['goal_step']
    print('%s: goal_step of the unretired run %s (N = %d)' % (what, goal.tolist(), N))
    assert ((goal >= 1) & (goal <= N - 10)).all(), goal            # the precondition: every ego arrives, well before the run ends
    fin, out = r['ret_final'], r['ret_out']
    assert (fin['done'] == 1).all()
    assert np.array_equal(fin['steps_driven'], goal) and np.array_equal(out['goal_step'], goal) and np.array_equal(out['steps'], goal)
    assert not fin['applied'].any()
    for q, g in enumerate(goal):
        a, b = r['plain_rows'][:g, q], r['ret_rows'][:g, q]
        _rows_same(a, b, '%s ego %d rows [0, %d)' % (what, q, g))
        last = b[g - 1]
        assert np.array_equal(fin['state'][q], [last['x'], last['y'], last['v'], last['yaw']]), (what, q)
        then = r['snaps'][g - 1]                                    # the unretired batch as it stood after step goal_step - 1
        assert np.array_equal(then['state'][q], fin['state'][q])
        for k in FROZEN:
            assert then[k][q].tobytes() == fin[k][q].tobytes(), (what, q, k)
        contact, minc = outcome_from_clearances(r['plain_rows']['clearance'][:g, q])
        assert out['contact_step'][q] == contact and out['min_clearance'][q] == minc, (what, q)
        # beyond its own cursor an agent has no rows: zeros in rows() for all agents
        assert not r['ret_rows'][g:, q].tobytes().strip(b'\0'), (what, q)
    assert len(r['ret_rows']) == goal.max()
    assert r['stats']['agent_steps'] == int(fin['steps_driven'].sum()), (r['stats'], fin['steps_driven'])
    assert r['stats']['iterations'] == int(sum(r['ret_rows']['iters'][:g, q].sum() for q, g in enumerate(goal)))
    # the scripted cars never noticed
    assert r['plain_final']['traffic_state'].tobytes() == fin['traffic_state'].tobytes()


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_single_ego_is_todays_loop_until_it_arrives(runs, mode):
    """Tests 1 and 4.  scripted_traffic_batch(B = 4, T = 13, A = 1, K = 2) with a log of capacity N, N steps without and with retirement
    (mode 'speed': stop_mode='speed' with lib.mpc_with_speed.params(), the goal tested against the whole path).  The ego meets only
    scripted cars, which never yield, so its trajectory up to its arrival cannot depend on retirement.  Per ego: log rows [0, goal_step)
    bit-identical; done == 1; steps_driven == goal_step == log.steps; final state == row goal_step - 1; applied == 0; sol, pre, inter,
    target_ind, traj_idx (and prev_len in speed mode) as the unretired batch held them after step goal_step - 1; min_clearance and
    contact_step from the unretired rows [0, goal_step) alone; agent-steps of the statistics == steps_driven.sum(); traffic_state after
    N steps bit-identical."""
    _assert_single_ego_parity(runs(mode), mode)


@pytest.mark.parametrize('solver', ['condensed', 'stage'])
def test_both_solvers(stock, solver):
    """Test 2.  Test 1 with the QP solver forced: the condensed kernel's queue-length test (it stops drawing tickets at the device-side
    count instead of at B) and the stage solver's are each exercised, and each solver's retired run is bit-identical to ITS unretired run
    up to every arrival (two solvers are two algorithms: their iterates agree to rounding, not bit for bit, so each is compared with
    itself)."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    try:
        c.set_qp_solver(solver)
        _assert_single_ego_parity(_runs(c, stock, 'cut'), solver)
    finally:
        c.close()


def test_graph_replay(runs, stock):
    """Test 3.  run(N, graph=True) with retirement on a side stream == run(N): every buffer, the log and done.  done, steps_driven and
    the queue length are device memory, so the one captured step retires agents as it is replayed."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    r = runs('cut')
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        g = _single(side, stock)
        lg = g.attach_log(N)
        g.retire_at_goal()
        torch.cuda.synchronize()
        g.run(N // 3, graph=True)
        g.run(N - N // 3, graph=True)
        _same(r['ret_final'], g.snapshot(), 'graph')
        _rows_same(r['ret_rows'], lg.rows(), 'graph')
        _same(r['ret_out'], lg.outcomes(), 'graph outcomes')
        assert (g.snapshot()['done'] == 1).all()
    finally:
        side.close()


def _coupled(c, stock, retire):
    """2 instances x 8 agents on the stock routes, all at their routes' starts (the second manoeuvre of an arm 8 m behind the first's start
    point, so that no two cars start on the same pose) but one per instance, which starts 10 m before the end of its route"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, MpcParams
    routes, dl, cd = stock
    B, A = 2, 8
    route = np.tile(np.arange(A) % len(routes), (B, 1))
    start = np.zeros((B, A), dtype=np.int64)
    start[:, 1::2] = int(round(8.0 / dl))
    # (agent 5, route (3, 2), in both: it arrives after 43 steps; from the same place on route (2, 1) a car has not arrived after 80)
    for b, k in ((0, 5), (1, 5)):
        start[b, k] = len(routes[route[b, k]]) - 1 - int(round(10.0 / dl))
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    sim = IntersectionBatch(c, MpcParams(T=13, L=cd.distance_back_to_front_wheel), ip, routes, dl, route, start)
    if retire:
        sim.retire_at_goal()
    return sim


def test_coupled_agents(ctx, stock):
    """Test 5.  Stepped with run(1) + snapshot() beside an unretired twin.  Precondition: at some step an agent is retired while another
    of its instance still drives.  Until the first arrival in an instance every buffer of that instance equals the twin's (in the step of
    the arrival all but the arrived agent's applied row, which is zeroed); from its retirement on every buffer of a retired agent is the
    same from snapshot to snapshot; its pool row is (x, y, v, yaw, 0, 0) of its frozen state; the driving agents' status stays 0; check()
    passes."""
    A, steps = 8, 80
    sim, twin = _coupled(ctx, stock, True), _coupled(ctx, stock, False)
    P = sim.P
    first = {}                  # instance -> step (1-based) of its first arrival
    prev = None
    mixed = False
    for s in range(1, steps + 1):
        sim.run(1); twin.run(1)
        a, t = sim.snapshot(), twin.snapshot()
        done = a['done'] != 0
        was = np.zeros(P, bool) if prev is None else prev['done'] != 0
        assert (a['status'][~was] == 0).all(), (s, a['status'])
        for b in range(P // A):
            sl = slice(b * A, (b + 1) * A)
            if b not in first and done[sl].any():
                first[b] = s
            if b not in first or first[b] == s:
                for k in PER_AGENT:
                    x, y = a[k][sl].copy(), t[k][sl].copy()
                    if k == 'applied' and b in first:
                        assert not x[done[sl]].any()
                        x[done[sl]], y[done[sl]] = 0, 0
                    assert x.tobytes() == y.tobytes(), (s, b, k)
            mixed |= bool(done[sl].any() and not done[sl].all())
        for q in np.nonzero(was)[0]:                               # retired before this step: frozen, and a parked car in the pool
            for k in PER_AGENT:
                assert prev[k][q].tobytes() == a[k][q].tobytes(), (s, q, k)
            assert a['steps_driven'][q] == prev['steps_driven'][q] and not a['applied'][q].any()
            row = sim.obs6[int(sim.obs_skip[q])].cpu().numpy()
            assert np.array_equal(row, np.concatenate([a['state'][q], [0.0, 0.0]])), (s, q, row)
        prev = a
    print('coupled: first arrivals %s, done after %d steps %s' % (first, steps, prev['done'].tolist()))
    assert mixed and len(first) == 2 and max(first.values()) <= steps - 10, first
    sim.check()
    assert sim.active_count() == P - int(prev['done'].sum()) > 0


def test_everything_retired(ctx, stock, runs):
    """Test 6.  With every ego of test 1's batch retired, run(5) changes no buffer of the agents and none of the log's and moves no
    statistic -- the scripted cars alone go on (traffic_state and their pool rows; `Other actors` of the semantics).
    run_until_done(200, chunk=16) on a fresh batch returns fewer than 200 steps with active_count() == 0."""
    r = runs('cut')
    sim, log = r['ret'], r['ret_log']
    assert sim.active_count() == 0
    before, rows, out = sim.snapshot(), log.rows(), log.outcomes()
    ctx.closed_loop_stats(reset=True)
    sim.run(5)
    after = sim.snapshot()
    _same(before, after, 'all retired', keys=PER_AGENT + ('done', 'steps_driven'))
    ego = sim.ego_row.cpu().numpy()
    assert before['obs6'][ego].tobytes() == after['obs6'][ego].tobytes()
    assert before['traffic_state'].tobytes() != after['traffic_state'].tobytes()
    _rows_same(rows, log.rows(), 'all retired')
    _same(out, log.outcomes(), 'all retired: outcomes')
    assert ctx.closed_loop_stats() == dict(agent_steps=0, iterations=0, failures=0, max_iterations=0)
    fresh = _single(ctx, stock)
    fresh.retire_at_goal()
    taken = fresh.run_until_done(200, chunk=16)
    goal = r['plain_out']['goal_step']
    print('run_until_done: %d steps for arrivals after %s' % (taken, goal.tolist()))
    assert taken < 200 and fresh.active_count() == 0
    assert taken == -(-int(goal.max()) // 16) * 16 and np.array_equal(fresh.steps_driven.cpu().numpy(), goal)


def test_refusals_and_keep_driving(ctx, stock):
    """Test 7.  MPCX_E_INVALID / MpcxError with nothing launched (the state is unchanged): one pointer of the struct null, a goal_dis that
    is not finite, two linearisation passes, step_staged().  An all-zero struct is no retirement; keep_driving() followed by run(3) on a
    batch that never arrived equals a batch that never had retirement, bit for bit."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim, never = _single(ctx, stock), _single(ctx, stock)
    sim.retire_at_goal()
    desc = sim._descriptor()
    before = sim.snapshot()

    def variant(**kw):
        c = _lib.RetireC()
        C.memmove(C.byref(c), C.byref(sim._retire), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    for bad in (variant(done=None), variant(steps_driven=None), variant(goal_dis=float('nan')), variant(goal_dis=float('inf')),
                variant(stop_speed=float('nan'))):
        for graph in (False, True):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=r'mpcx error -1: retire'):
                    ctx.closed_loop_run(sim.ip, desc, n, graph, retire=bad)
    ctx.set_linearisation_passes(2)
    try:
        with pytest.raises(MpcxError, match=r'mpcx error -1: retire: 2 linearisation passes'):
            ctx.closed_loop_run(sim.ip, desc, 1, retire=sim._retire)
    finally:
        ctx.set_linearisation_passes(1)
    sim.lin_passes = 2
    with pytest.raises(MpcxError, match='lin_passes = 2'):
        sim.run(1)
    sim.lin_passes = 1
    with pytest.raises(MpcxError, match='step_staged'):
        sim.step_staged()
    with pytest.raises(MpcxError, match='differ from'):
        sim.attach_log(4, goal_dis=2.0)
    _same(before, sim.snapshot(), 'refused')
    assert sim.steps_done == 0 and not sim.steps_driven.any()
    # an all-zero struct: the plain run
    ctx.closed_loop_run(sim.ip, desc, 2, retire=_lib.RetireC())
    never.run(2)
    _same(never.snapshot(), sim.snapshot(), 'all-zero struct', keys=never.snapshot().keys())
    assert not sim.steps_driven.any()
    # retirement on for a few steps in which nobody arrives, then off again
    sim.run(4); never.run(4)
    assert sim.active_count() == sim.P and (sim.steps_driven.cpu().numpy() == 4).all()
    sim.keep_driving()
    sim.run(3); never.run(3)
    a, b = sim.snapshot(), never.snapshot()
    assert 'done' not in a
    _same(b, a, 'keep_driving')
