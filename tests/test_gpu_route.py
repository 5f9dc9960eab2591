"""GPU tests of ROUTES in the device-resident closed loop (mpcx_closed_loop_run_routes, IntersectionBatch.respawn_on_schedule(route=...)):
every vehicle of a respawning slot takes its own route from its own start pose, written on the device by the reset that hands the slot to
the admission gate.  The defining properties: a routed vehicle starts exactly like the first vehicle of a fresh batch on that route (its log
rows repeat that batch's bit for bit), and a run with device routing equals, bit for bit, a run with admission alone whose words -- path_off
and path_len included -- the host build of the rule (tests/route_ref) rewrites between run(1) calls, while every driving agent of every step
equals the oracle step over the present rows.  Then: graph replay, off means off, the refusals and the per-movement summary.  The host build
of the rule is tests/test_route_cpu.py.

The scene of the twins, tried on the CPU oracle alone first (tests/route_helpers.RouteOracleLoop): two arms with two slots each yield to each
other a lot -- in 240 steps instance 0 sees five arrivals in cut mode (steps 84, 117, 158, 186, 233) and instance 1 three."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import admit_helpers as AH
from tests import respawn_helpers as RH
from tests import route_helpers as TH
from tests import test_gpu_respawn as GR
from tests import test_gpu_scene as GS

pytestmark = pytest.mark.gpu

T = GR.T
ROUTE0 = np.tile(np.arange(4), (2, 1))                      # B = 2, A = 4: arms 1 and 2, two slots each, both at one start pose
START0 = np.array([[180] * 4, [170] * 4])                   # (the two stock routes of an arm share their first 181 points)
DUE = np.tile(np.array([[0, 10, 60], [5, 20, 30], [0, 15, 40], [8, 20, 50]]), (2, 1, 1))
SHARE = [1, 2, 2, 1, 1, 1, 1, 1]
STEPS = 240
LOG_WORDS = GR.LOG_WORDS


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
    d = tmp_path_factory.mktemp('route_ref')
    return types.SimpleNamespace(admit=AH.build_ref(d), respawn=RH.build_ref(d), route=TH.build_ref(d))


def _demand(stock):
    from mpc_for_av_at_intersection_amd.batch import turning_demand
    return turning_demand(ROUTE0, stock[0], START0, SHARE, 3, seed=3)


def _routed(ctx, stock, mode='cut', log=0):
    """the B = 2 batch with routes from turning_demand"""
    sim = GR._batch(ctx, stock, ROUTE0, START0, mode)
    if log:
        sim.attach_log(log)
    sim.respawn_on_schedule(DUE, gap=1.0, route=_demand(stock))
    return sim


class HandDriven(GR.HandDriven):
    """the twin: a batch with ADMISSION ONLY, and the host build of the ROUTED rule applied to its device words -- path_off and path_len
    among them -- with torch copies after every run(1)"""

    def __init__(self, libs, sim, routes, due, gap, route, start_idx):
        super().__init__(libs, sim, due, gap)
        c = self.case
        lens = np.array([len(r) for r in routes])
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        route, start_idx = np.asarray(route).reshape(sim.P, -1), np.asarray(start_idx).reshape(sim.P, -1)
        rstate = np.zeros((sim.P, c.G, 4))
        for q in range(sim.P):
            for g in range(c.G):
                p = routes[route[q, g]][start_idx[q, g]]
                rstate[q, g] = [p[0], p[1], 0.0, p[2]]
        words = {k: getattr(c, k) for k in RH.MUT_F64 + RH.MUT_I32 + RH.CONST_I32 + ('start_state',)}
        self.case = TH.Case(c.P, T, c.G, c.n_pool, len(routes), log=c.log, speed=c.speed, route_off=offs, route_len=lens, route_of=route,
                            rstart_idx=start_idx, rstart_state=rstate, path_off=sim.path_off.cpu().numpy(), path_len=sim.path_len.cpu().numpy(),
                            **words)

    def respawn(self):
        sim, c = self.sim, self.case
        sim.ctx.synchronize()
        dev = dict(GR._words(sim), path_off=sim.path_off, path_len=sim.path_len)
        for k, t in dev.items():
            getattr(c, k)[...] = t.cpu().numpy().reshape(getattr(c, k).shape)
        c.done[...] = sim.done.cpu().numpy()
        c.clock[...] = sim.clock.cpu().numpy()
        if TH.host_step(self.libs.route, c):
            for k, t in dev.items():
                t.copy_(torch.from_numpy(getattr(c, k).reshape(tuple(t.shape))).to(t.device))
            sim.ctx.synchronize()


# ---------------------------------------------------------------- T1
def test_stage_alone(ctx, libs):
    """T1.  Context.respawn_step(routes=...) on the hand-made words of tests/test_route_cpu.py repeated to P = 65 -- two blocks, the second
    with one lane --, with and without log words, with and without prev_len, gives the bytes of the host build; so does a second step on the
    device's own words.  P = 0 is a no-op."""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    arrived = 0
    names = RH.MUT_F64 + RH.MUT_I32 + RH.CONST_I32 + ('start_state',) + TH.ROUTE_I32 + ('path_off', 'path_len', 'rstart_state')
    for log, speed in ((True, False), (False, False), (True, True), (False, True)):
        host = TH.hand_made(log, speed, P=65)
        ctx.set_mpc_params(MpcParams(T=host.T, L=2.86))
        dev = types.SimpleNamespace(G=host.G, R=host.R, log=log, **{k: torch.from_numpy(getattr(host, k).copy()).to(ctx.device) for k in names})
        for step in range(2):
            lg, retire, admit, rs, rt = TH.structs(dev, ptr=lambda t: t.data_ptr())
            ctx.respawn_step(dev.state, dev.applied, dev.u.view(host.P, 2, host.T), dev.traj_idx, dev.target_ind, dev.cut_len, dev.iters, dev.own,
                             host.n_pool, retire, admit, rs, prev_len=dev.prev_len if speed else None, log=lg, routes=rt, max_path_len=1024)
            ctx.synchronize()
            arrived += TH.host_step(libs.route, host)
            for k in TH.MUT_F64 + TH.MUT_I32:
                assert getattr(dev, k).cpu().numpy().tobytes() == getattr(host, k).tobytes(), (log, speed, step, k)
            host.clock[0] += 1
            dev.clock += 1
    assert arrived == 4 * len([q for q in range(65) if q % 9 in TH.ARRIVE])
    # nobody: nothing is launched, nothing is read
    e = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=ctx.device)
    i32, f64 = torch.int32, torch.float64
    ctx.respawn_step(e(f64, 0, 4), e(f64, 0, 2), e(f64, 0, 2, host.T), e(i32, 0), e(i32, 0), e(i32, 0), e(i32, 0), e(i32, 0), 0, retire, admit, rs,
                     routes=rt, max_path_len=1024)
    ctx.synchronize()
    for k in TH.MUT_F64 + TH.MUT_I32:
        assert getattr(dev, k).cpu().numpy().tobytes() == getattr(host, k).tobytes(), k


# ---------------------------------------------------------------- T2
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_a_routed_vehicle_starts_like_a_fresh_one_on_its_route(ctx, stock, mode):
    """T2.  B = 1, A = 1, G = 3 on the stock routes r0, r1, r0 = (1, 1), (1, 2), (1, 1), each from index len(route) - 120, due all 0, a log
    of 96 rows.  The log rows of vehicle 2 equal, bit for bit and in all 16 columns, the first-vehicle rows of a FRESH UNROUTED batch on r1
    from that index; vehicle 3's equal vehicle 1's, which equal those of a fresh unrouted batch on r0.  A word the routed reset forgot
    would show here."""
    routes = stock[0]
    order = [0, 1, 0]
    start = [len(routes[r]) - 120 for r in order]

    def rows_of(sim, log):
        ep = sim.episodes()
        f, w = log.rows_f64.cpu().numpy(), log.rows_i32.cpu().numpy()
        return ep, [(f[b:e, 0].copy(), w[b:e, 0].copy()) for b, e in zip(ep['row_begin'], ep['row_end'])]
    sim = GR._batch(ctx, stock, [[order[0]]], [[start[0]]], mode)
    log = sim.attach_log(96)
    sim.respawn_on_schedule(np.zeros((1, 1, 3), dtype=np.int64), gap=0.0, route=[[order]], start_index=[[start]])
    assert sim.snapshot()['route'].tolist() == [0]
    seen = []
    for _ in range(80):
        sim.run(1)
        seen.append(int(sim.snapshot()['route'][0]))
    ep, rows = rows_of(sim, log)
    print(mode, ep, sim.episode_routes())
    assert sim.served_count() == 3 and sim.episode_routes().tolist() == order and set(seen) == {0, 1} and seen[-1] == 0
    assert (ep['arrived'] - ep['entered'] + 1 == ep['steps_driven']).all() and ep['steps_driven'].min() > 5
    assert ep['entered'].tolist() == [0] + (ep['arrived'][:2] + 1).tolist()
    for r in (0, 1):
        fresh = GR._batch(ctx, stock, [[r]], [[len(routes[r]) - 120]], mode)
        flog = fresh.attach_log(96)
        fresh.respawn_on_schedule(np.zeros((1, 1, 1), dtype=np.int64), gap=0.0)
        fresh.run(40)
        fep, frows = rows_of(fresh, flog)
        assert fresh.served_count() == 1 and fep['entered'][0] == 0
        for g in [g for g in range(3) if order[g] == r]:
            assert ep['steps_driven'][g] == fep['steps_driven'][0], (r, g)
            assert rows[g][0].tobytes() == frows[0][0].tobytes() and rows[g][1].tobytes() == frows[0][1].tobytes(), (r, g)
    assert rows[0][0].tobytes() == rows[2][0].tobytes() and rows[0][0].tobytes() != rows[1][0].tobytes()
    sim.ctx.synchronize()
    assert sim.path_off.cpu().tolist() == [0] and sim.path_len.cpu().tolist() == [len(routes[0])]


# ---------------------------------------------------------------- T3
def _pair_of_runs(ctx, libs, stock, mode, steps, log=0):
    """X with respawn_on_schedule(route=...) beside its hand-driven twin Y for `steps` steps of run(1); after every step every snapshot key
    of Y must be X's bit for bit, as must path_off, path_len, wait, entered_step, served, the episode table and the log's outcome words;
    and every driving agent equals the oracle step over the present rows"""
    route = _demand(stock)
    start_idx = np.repeat(START0[:, :, None], 3, axis=2)
    X = _routed(ctx, stock, mode, log)
    Ysim = GR._batch(ctx, stock, ROUTE0, START0, mode)
    if log:
        Ysim.attach_log(log)
    # vehicle 0 of every slot on ITS route (the twin has no routes: its constructor's route is not the first vehicle's)
    r0 = route[:, :, 0].reshape(-1)
    Ysim.path_off.copy_(ctx.i32(Ysim._route_offs[r0])); Ysim.path_len.copy_(ctx.i32(np.diff(Ysim._route_offs)[r0]))
    Y = HandDriven(libs, Ysim, stock[0], DUE, 1.0, route, start_idx)
    worst = 0.0
    for s in range(steps):
        X.run(1)
        before = Ysim.snapshot()
        before, gate = Y.admitted(before)
        Ysim.run(1)
        after = Ysim.snapshot()
        assert np.array_equal(after['wait'], gate.wait) and np.array_equal(after['entered_step'], gate.entered), s
        w, _ = GS._replay_step(Ysim, before, after, GS._pool_before(Ysim, before, after), before['absent'])
        worst = max(worst, w)
        Y.respawn()
        x, y = X.snapshot(), Ysim.snapshot()
        assert sorted(x) == sorted(list(y) + ['served', 'route'])
        for k in y:
            assert x[k].tobytes() == y[k].tobytes(), (s, k)
        c = Y.case
        for k in ('path_off', 'path_len'):
            assert getattr(X, k).cpu().numpy().tobytes() == getattr(Ysim, k).cpu().numpy().tobytes() == getattr(c, k).tobytes(), (s, k)
        assert np.array_equal(x['served'], c.served) and int(X.clock.item()) == s + 1 == int(Ysim.clock.item()), s
        assert X.ep_i32.cpu().numpy().tobytes() == c.ep_i32.tobytes() and X.ep_f64.cpu().numpy().tobytes() == c.ep_f64.tobytes(), s
        if log:
            for k in LOG_WORDS:
                assert getattr(X.log, k).cpu().numpy().tobytes() == getattr(Ysim.log, k).cpu().numpy().tobytes(), (s, k)
    if log:
        assert X.log.rows_f64.cpu().numpy().tobytes() == Ysim.log.rows_f64.cpu().numpy().tobytes()
        assert X.log.rows_i32.cpu().numpy().tobytes() == Ysim.log.rows_i32.cpu().numpy().tobytes()
    return types.SimpleNamespace(X=X, Y=Y, worst=worst, route=route)


@pytest.fixture(scope='module', params=['cut', 'speed'])
def twins(request, ctx, libs, stock):
    return request.param, _pair_of_runs(ctx, libs, stock, request.param, STEPS, log=STEPS)


def test_device_rule_equals_the_host_rule(twins):
    """T3.  B = 2, A = 4 (two arms x two slots, one start pose per arm), G = 3, routes from turning_demand, gap 1 m, 240 steps, both stop
    modes: after every step every snapshot key, path_off, path_len, wait, entered_step, served, the episode table and the log's words of
    the device run equal those of the twin that has admission only and whose words the host build of the rule rewrites between steps; every
    driving agent of every step equals the oracle step over the present rows within 2e-7 -- all asserted while the fixture ran.  Here:
    vehicles did change route, and every finished episode carries its route."""
    mode, r = twins
    ep, er = r.X.episodes(), r.X.episode_routes()
    print('%s: worst |GPU - oracle| %.2e over %d steps; %d episodes, routes %s' % (mode, r.worst, STEPS, len(ep), er.tolist()))
    assert len(ep) >= 6 and (ep['arrived'] - ep['entered'] + 1 == ep['steps_driven']).all() and (ep['delay'] >= 0).all()
    flat = r.route.reshape(-1, 3)
    assert er.tolist() == [int(flat[q, g]) for q, g in zip(ep['slot'], ep['generation'])]
    assert (er // 2 == (ep['slot'] % 4) // 2).all()             # every vehicle stayed on its arm
    served = r.X.snapshot()['served']
    now = r.X.snapshot()['route']
    moved = [q for q in range(8) if len(set(flat[q, :min(int(served[q]), 2) + 1].tolist())) > 1]
    assert moved and all(now[q] == flat[q, served[q]] for q in range(8) if served[q] < 3)


# ---------------------------------------------------------------- T4
def test_graph_replay_and_chunking(ctx, stock):
    """T4.  T3's batch as 30 chunks of run(7, graph=True) equals 210 x run(1) plain, byte for byte: the final snapshot, episodes(), the
    episode table and path_off / path_len."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _routed(ctx, stock)
    for _ in range(210):
        plain.run(1)
    a = plain.snapshot()
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = GR._batch(side, stock, ROUTE0, START0)
        graph.respawn_on_schedule(DUE, gap=1.0, route=_demand(stock))
        torch.cuda.synchronize()
        for _ in range(30):
            graph.run(7, graph=True)
        b = graph.snapshot()
        assert sorted(a) == sorted(b) and 'route' in a
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert int(graph.clock.item()) == 210 == int(plain.clock.item())
        assert plain.episodes().tobytes() == graph.episodes().tobytes() and len(plain.episodes()) >= 5
        for k in ('ep_i32', 'ep_f64', 'path_off', 'path_len'):
            assert getattr(plain, k).cpu().numpy().tobytes() == getattr(graph, k).cpu().numpy().tobytes(), k
        assert len(set(plain.episode_routes().tolist())) > 1
    finally:
        side.close()


# ---------------------------------------------------------------- T5
def _entry(sim, routes, n, respawn='own'):
    """mpcx_closed_loop_run_routes itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    rs = sim._respawn if isinstance(respawn, str) else respawn
    ref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_routes(c._ctx, C.byref(cip), C.byref(sim._desc), None, ref(sim._opts), ref(sim._retire), ref(sim._scene),
                                             ref(sim._admit), ref(rs), ref(routes), int(n), 0))


def test_off_means_off(ctx, stock):
    """T5a.  route=None, routes = NULL and an all-zero routes struct each give the bytes of the respawn run -- 60 steps of the first
    instance of tests/test_gpu_respawn.py's queue, two arrivals and two resets included; path_off and path_len never move."""
    from mpc_for_av_at_intersection_amd import _lib
    due = np.array([GR.DUE2])

    def fresh():
        sim = GR._batch(ctx, stock, GR.ROUTE3[:1], GR.START3[:1])
        sim.respawn_on_schedule(due, gap=1.0)
        return sim
    base = fresh()
    off0, len0 = base.path_off.cpu().numpy().copy(), base.path_len.cpu().numpy().copy()
    c = base.ctx
    base._claim_context()
    base._desc = base._descriptor()
    cip = base.ip.to_c()
    c._chk(c.lib.mpcx_closed_loop_run_respawn(c._ctx, C.byref(cip), C.byref(base._desc), None, None, C.byref(base._retire), C.byref(base._scene),
                                              C.byref(base._admit), C.byref(base._respawn), 60, 0))
    want, want_ep = base.snapshot(), base.ep_i32.cpu().numpy().tobytes()
    assert want['served'].tolist() == [1, 1] and 'route' not in want
    runs = {}
    sim = fresh(); assert sim._routes is None; sim.run(60); runs['route=None'] = sim
    sim = fresh(); _entry(sim, None, 60); runs['NULL'] = sim
    sim = fresh(); _entry(sim, _lib.RoutesC(), 60); runs['zero struct'] = sim
    for name, sim in runs.items():
        got = sim.snapshot()
        assert sorted(got) == sorted(want), name
        for k in want:
            assert want[k].tobytes() == got[k].tobytes(), (name, k)
        assert sim.ep_i32.cpu().numpy().tobytes() == want_ep, name
        assert np.array_equal(sim.path_off.cpu().numpy(), off0) and np.array_equal(sim.path_len.cpu().numpy(), len0), name
    assert not base.ep_i32.cpu().numpy()[:, :, 7].any()


def test_refusals(ctx, stock):
    """T5b.  MPCX_E_INVALID with a "routes: ..." message before anything is launched, whatever n_steps is, and every buffer unchanged: routes
    without respawn, each of the seven pointers missing, n_routes < 1, path_off / path_len that are not the descriptor's, a route_len below
    1 or above the interaction parameters' effective max_path_len.  In Python: bad route / start_index arrays raise ValueError before
    anything changes; stop_respawning(), enter_now() and keep_driving() drop routing together with respawn."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _routed(ctx, stock)
    words = lambda: dict(sim.snapshot(), path_off=sim.path_off.cpu().numpy(), path_len=sim.path_len.cpu().numpy(), ep=sim.ep_i32.cpu().numpy())
    before = words()
    rt = sim._routes
    good = [rt.n_routes, 0, rt.route_off, rt.route_len, rt.route_of, rt.start_state, rt.start_idx, rt.path_off, rt.path_len]
    R = rt.n_routes
    lens = sim.route_len.cpu().numpy()
    cap = (max(int(sim.ip.max_path_len), 512) + 63) // 64 * 64
    assert lens.max() <= cap
    other = torch.zeros(sim.P, dtype=torch.int32, device=ctx.device)
    short, long_ = ctx.i32(np.where(np.arange(R) == 2, 0, lens)), ctx.i32(np.where(np.arange(R) == 5, cap + 1, lens))
    for n in (0, 3):
        with pytest.raises(MpcxError, match='routes: routes need respawn'):
            _entry(sim, rt, n, respawn=None)
        with pytest.raises(MpcxError, match='routes: routes need respawn'):
            _entry(sim, rt, n, respawn=_lib.RespawnC())
        for i, name in enumerate(('route_off', 'route_len', 'route_of', 'start_state', 'start_idx', 'path_off', 'path_len')):
            bad = list(good); bad[2 + i] = None
            with pytest.raises(MpcxError, match='routes: .*%s is null' % name):
                _entry(sim, _lib.RoutesC(*bad), n)
        for r in (0, -2):
            with pytest.raises(MpcxError, match='routes: n_routes'):
                _entry(sim, _lib.RoutesC(r, *good[1:]), n)
        for i in (7, 8):
            bad = list(good); bad[i] = other.data_ptr()
            with pytest.raises(MpcxError, match='routes: path_off and path_len must be the descriptor'):
                _entry(sim, _lib.RoutesC(*bad), n)
        for tab, r, v in ((short, 2, 0), (long_, 5, cap + 1)):
            bad = list(good); bad[3] = tab.data_ptr()
            with pytest.raises(MpcxError, match='routes: route %d has %d points' % (r, v)):
                _entry(sim, _lib.RoutesC(*bad), n)
    after = words()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert int(sim.clock.item()) == 0 and sim.served_count() == 0 and not other.any()
    route = _demand(stock)
    for kw in (dict(route=route[:, :, :2]), dict(route=route.astype(np.float64)), dict(route=route + 7), dict(route=-route - 1),
               dict(route=route, start_index=np.full((2, 4, 3), 720)), dict(route=route, start_index=np.full((2, 4, 2), 5)),
               dict(start_index=np.zeros((2, 4, 3), dtype=np.int64))):
        with pytest.raises(ValueError):
            sim.respawn_on_schedule(DUE, gap=1.0, **kw)
    late = GR._batch(ctx, stock, [[0, 2]], [[700, 600]])         # the default start index, 700, lies outside route 2 (660 points)
    with pytest.raises(ValueError, match='current traj_idx'):
        late.respawn_on_schedule(np.zeros((1, 2, 2), dtype=np.int64), route=[[[0, 2], [2, 3]]])
    assert late._respawn is None and late._admit is None
    after = words()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    for off in ('stop_respawning', 'enter_now', 'keep_driving'):
        sim = _routed(ctx, stock)
        assert 'route' in sim.snapshot()
        getattr(sim, off)()
        assert sim._routes is None and sim._respawn is None and 'route' not in sim.snapshot()


# ---------------------------------------------------------------- T6
def test_movement_summary(ctx, stock, twins):
    """T6.  movement_summary() -- the table reduced on the device -- equals the numpy definition (route_helpers.summary_numpy) exactly, field
    by field and byte for byte, on T3's B = 2 run; its counts add up to the episodes and split as episode_routes() says.  An all-empty
    table (a fresh batch) gives zeros and +inf."""
    mode, r = twins
    X = r.X
    got = X.movement_summary()
    want = TH.summary_numpy(X.A, 8, X.served.cpu().numpy(), X.ep_i32.cpu().numpy(), X.ep_f64.cpu().numpy())
    print(mode, got)
    assert got.shape == (2, 8) and got.dtype == want.dtype
    for n in got.dtype.names:
        assert got[n].tobytes() == want[n].tobytes(), n
    ep, er = X.episodes(), X.episode_routes()
    assert got['count'].sum() == len(ep) >= 6
    for b in range(2):
        for k in range(8):
            sel = (ep['slot'] // 4 == b) & (er == k)
            assert got['count'][b, k] == sel.sum() and got['delay_sum'][b, k] == ep['delay'][sel].sum()
            assert got['min_clearance'][b, k] == (ep['min_clearance'][sel].min() if sel.any() else np.inf)
    assert not got['count'][:, 4:].any()
    fresh = _routed(ctx, stock, mode)
    empty = fresh.movement_summary()
    assert empty.shape == (2, 8) and np.isinf(empty['min_clearance']).all() and (empty['min_clearance'] > 0).all()
    for n in ('count', 'contacts', 'delay_sum', 'steps_driven_sum'):
        assert not empty[n].any(), n
