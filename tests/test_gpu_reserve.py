"""GPU tests of CROSSING RESERVATIONS in the device-resident closed loop (mpcx_closed_loop_run_reserved, mpcx_reserve_step_batch,
IntersectionBatch.reserve): reserve_kernel takes the place of signal_kernel -- a lane group per junction classifies the junction's agents,
grants the requests in order by a loop of group-wide minima and holds the others with the signal rule's own hold.  The stage call against
the host build of the rule on the hand-made junctions of tests/test_reserve_cpu.py at every lane-group size; the closed loop against
ReserveOracleLoop with two managers in one batch; graph replay, host staging, off means off, the refusals.  B = 2, A = 4, T = 13, v0 = 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import reserve_helpers as RH
from tests import signal_helpers as G
from tests import test_gpu_respawn as GR

pytestmark = pytest.mark.gpu

STRAIGHT = np.tile(np.array([1, 3, 5, 7]), (2, 1))         # the four straight stock routes
TURN1 = np.tile(np.array([0, 2, 4, 6]), (2, 1))            # the four (arm, 1) stock routes
PATIENCE = (0, None)                                        # instance 0 strict first come, first served; instance 1 first fit
DETECT = 144                                                # the stock routes' line index: the detector is the whole approach


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
    return RH.build_ref(tmp_path_factory.mktemp('reserve_ref'))


def _managers():
    return [dict(detect=DETECT, patience=p) for p in PATIENCE]


def _scene(c, stock, routes=STRAIGHT, reserved=True, retire=True):
    """B = 2 instances of four stock routes from index 0, cut mode; instance b under manager b"""
    sim = GR._batch(c, stock, routes, np.zeros((2, 4), dtype=np.int64), 'cut')
    if not retire:
        sim.keep_driving()
    if reserved:
        sim.reserve(_managers(), manager_of=np.array([0, 1]))
    return sim


def _snap(sim):
    out = sim.snapshot()
    if sim._reservation is not None:
        out['queued'], out['clock'] = sim.queued.cpu().numpy().copy(), sim.junction_clock.cpu().numpy().copy()
    return out


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in b:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---------------------------------------------------------------- GR1
def _device_stage(c, w):
    """mpcx_reserve_step_batch on the words of reserve_helpers.words(); returns OUT_KEYS as the device left them"""
    from mpc_for_av_at_intersection_amd import _lib
    d = {k: c.i32(w[k]) for k in RH.I32_KEYS}
    state = c.f64(w['state'])
    done = None if w['done'] is None else c.i32(w['done'])
    sg = _lib.SignalsC(d['path_stop'].data_ptr(), d['path_group'].data_ptr(), None, None, None, None, None, d['held'].data_ptr(), float(w['brake']),
                       len(w['path_stop']), 0, int(w['n_groups']), 0)
    rv = _lib.ReservationC(d['path_exit'].data_ptr(), d['conflict'].data_ptr(), d['lane'].data_ptr(), d['mgr_time'].data_ptr(),
                           d['mgr_of'].data_ptr(), d['grant'].data_ptr(), d['since'].data_ptr(), d['clock'].data_ptr(), d['occupied'].data_ptr(),
                           d['queued'].data_ptr(), int(w['n_per']), len(w['mgr_of']), len(w['mgr_time']), 0)
    c.synchronize()
    c.reserve_step(float(w['dl']), state, d['path_off'], d['path_len'], d['traj_idx'], d['cut_len'], sg, rv, done=done)
    c.synchronize()
    got = {k: d[k].cpu().numpy() for k in RH.I32_KEYS}
    for k in RH.I32_KEYS:       # nothing but the outputs is written
        if k not in RH.OUT_KEYS:
            assert got[k].tobytes() == w[k].tobytes(), k
    assert state.cpu().numpy().tobytes() == w['state'].tobytes()
    return {k: got[k] for k in RH.OUT_KEYS}


@pytest.mark.parametrize('n_per,J', [(1, None), (3, None), (8, None), (64, None), (8, 1), (8, 33)], ids=lambda v: 'all' if v is None else str(v))
def test_stage_call_equals_the_host_build(ctx, ref, n_per, J):
    """GR1.  mpcx_reserve_step_batch on the hand-made junctions equals the host build byte for byte -- grant, since, clock, occupied,
    queued, held, cut_len -- and the values written down by hand, with and without the retirement words: n_per = 1 (a lane per junction,
    no shuffle), 3 (a padding lane in every group of 4), 8, 64 (a wavefront per junction, with the junctions of 64 requesters: 64 rounds of
    the grant loop); one junction alone (the aged requester that blocks); 33 junctions of 8 = five wavefronts, the last with one live
    group of eight."""
    w, want = RH.hand_made(n_per, repeat=2 if J == 33 else 1)
    if J == 1:
        j0 = next(i for i, c in enumerate(RH.CASES) if c[0].startswith('an aged denied requester'))
        w = RH.junctions(w, j0, j0 + 1)
    elif J is not None:
        w = RH.junctions(w, 0, J)
    assert J is None or len(w['mgr_of']) == J
    for with_done in (True, False):
        host = RH.copy_words(w)
        if not with_done:
            host['done'] = None
        got = _device_stage(ctx, host)
        n = RH.host_rule(ref, host)
        for k in RH.OUT_KEYS:
            assert got[k].tobytes() == host[k].tobytes(), (k, with_done, np.flatnonzero(got[k] != host[k]))
        assert n == int((got['held'] != 0).sum())
        if with_done and J is None:
            RH.check_against_want(dict(got), want, w)
    if J == 1:
        assert got['queued'].tolist() == [2] and got['occupied'].tolist() == [8]


# ---------------------------------------------------------------- GR2, GR3
def _sync(loop, before, rows):
    """the oracle loop's continuous words from the device's before the step (the integers -- held, grant, since, clock -- run on their own)"""
    loop.state, loop.applied = before['state'][rows].copy(), before['applied'][rows].copy()
    loop.traj_idx, loop.target = [int(v) for v in before['traj_idx'][rows]], [int(v) for v in before['target_ind'][rows]]
    loop.prev = [int(v) for v in before['prev_cut'][rows]]
    loop.u = [before['u'][p].copy() for p in rows]


def _replay(sim, loops, n_steps):
    """n_steps of `sim` (or fewer, once everybody has arrived), every one replayed on one ReserveOracleLoop per instance from the device's
    own state before the step; returns (worst |GPU - oracle|, held steps per agent, arrival steps, the last snapshot, steps run)"""
    P = sim.P
    worst, held_steps, arr = 0.0, np.zeros(P, dtype=np.int64), np.full(P, -1)
    for s in range(n_steps):
        before = _snap(sim)
        sim.run(1)
        after = _snap(sim)
        for b, loop in enumerate(loops):
            rows = list(range(4 * b, 4 * b + 4))
            assert [bool(d) for d in before['done'][rows]] == loop.done and [bool(d) for d in before['absent'][rows]] == loop.absent, (s, b)
            if all(loop.done):
                continue
            _sync(loop, before, rows)
            out = loop.step()
            assert (after['occupied'][b], after['queued'][b], after['clock'][b]) == (loop.occupied_hist[-1], loop.queued_hist[-1], loop.clock[0]), \
                (s, b, after['occupied'][b], after['queued'][b], loop.occupied_hist[-1], loop.queued_hist[-1])
            assert after['granted'][rows].tolist() == loop.grant.tolist() and after['since'][rows].tolist() == loop.since.tolist(), (s, b)
            assert after['held'][rows].tolist() == loop.held, (s, b)
            for a, p in enumerate(rows):
                r = out[a]
                if r is None:
                    assert before['done'][p] and after['held'][p] == 0 and after['granted'][p] == 0
                    continue
                want = (r['traj_idx'], r['cut'], r['target'], r['hit'], r['status'], r['held'], r['grant'], r['since'])
                got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p],
                       after['granted'][p], after['since'][p])
                assert want == tuple(int(v) for v in got), (s, p, want, got)
                worst = max(worst, float(np.abs(r['u_sol'] - after['u'][p]).max()), float(np.abs(r['x_sol'] - after['x'][p]).max()),
                            float(np.abs(r['post'] - after['state'][p]).max()))
                held_steps[p] += r['held'] != 0
                assert bool(after['done'][p]) == loop.done[a], (s, p)
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        if after['done'].all():
            break
    return worst, held_steps, arr, after, s + 1


def _loops(name):
    paths, dl, start, stop, group, ex, conflict, lane = RH.scene_tables(name)
    return [RH.ReserveOracleLoop(paths, dl, start, stop, group, ex, conflict, lane, DETECT, p, T=13, depart=True) for p in PATIENCE]


def test_straight_scene_on_the_oracle(ctx, stock):
    """GR2.  The straight scene, cut mode, departure on, instance 0 with patience 0 and instance 1 unbounded, until everybody has arrived.
    Every step is replayed on one ReserveOracleLoop per instance from the device's own state before the step (the loop's integers -- held,
    grant, since, clock -- are never re-synchronised).  grant, since, occupied, queued, clock, held, cut_len, traj_idx, target index, hit
    and status are identical; states and solutions agree within the 2e-7 of tests/test_gpu_actuated.py GA2.  Not vacuous: agents are held
    and released, and the two managers give different runs (first fit never holds arms 1 and 3)."""
    sim = _scene(ctx, stock)
    loops = _loops('straight')
    worst, held_steps, arr, after, n = _replay(sim, loops, 260)
    print('reserved straight scene: worst |GPU - oracle| %.2e over %d steps, arrivals %s, held steps %s' % (worst, n, arr.tolist(), held_steps.tolist()))
    assert worst < 2e-7, worst
    assert after['done'].all() and after['absent'].all() and not after['held'].any() and not after['granted'].any()
    assert arr[:4].tolist() == loops[0].arrival and arr[4:].tolist() == loops[1].arrival and arr[:4].tolist() != arr[4:].tolist()
    assert (held_steps[[1, 2, 3, 5, 7]] > 10).all() and not held_steps[[0, 4, 6]].any()
    assert all(lp.mixed_steps == [] and len(lp.grants) == 4 for lp in loops)


def test_left_turns_on_the_oracle(ctx, stock):
    """GR3.  The four (arm, 1) routes -- the scene that never clears when everybody yields -- for 60 steps, replayed the same way: the
    first car is through its turn and the others are served in their order, identically on the device and on the oracle."""
    sim = _scene(ctx, stock, TURN1)
    loops = _loops('turn1')
    worst, held_steps, arr, after, n = _replay(sim, loops, 60)
    print('reserved left turns: worst |GPU - oracle| %.2e over %d steps, arrivals %s, held steps %s, occupied %s' %
          (worst, n, arr.tolist(), held_steps.tolist(), after['occupied'].tolist()))
    assert worst < 2e-7, worst
    assert n == 60 and held_steps.max() > 10 and after['granted'].any() and after['occupied'].all()
    assert arr[4] == loops[1].arrival[0] > 0 and held_steps[:4].tolist() != held_steps[4:].tolist()


# ---------------------------------------------------------------- GR4
def test_graph_replay_and_host_staging(ctx, stock):
    """GR4.  15 chunks of run(7, graph=True) on a side stream equal 105 x run(1) plain, byte for byte, grant, since, clock, occupied,
    queued and held included: the manager's words live in device memory, so the one captured step keeps counting.  step_staged() -- the
    per-stage entry points with mpcx_reserve_step_batch between the conflict search and the window stage -- equals run(1) after every one
    of 40 steps on the plain loop without retirement."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _scene(ctx, stock)
    seen = set()
    for _ in range(105):
        plain.run(1)
        seen.add(tuple(plain.occupied.cpu().numpy().tolist()))
    a = _snap(plain)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _scene(side, stock)
        torch.cuda.synchronize()
        for _ in range(15):
            graph.run(7, graph=True)
        _same(a, _snap(graph), 'graph')
        assert len(seen) >= 3 and a['done'].any() and a['clock'].tolist() == [105, 105]
    finally:
        side.close()
    X, Y = (_scene(ctx, stock, retire=False) for _ in range(2))
    held = np.zeros(8, dtype=np.int64)
    for s in range(40):
        X.run(1); Y.step_staged()
        x = _snap(X)
        _same(x, _snap(Y), s)
        held += x['held'] != 0
    assert (held[[1, 2, 3, 5, 7]] > 10).all() and not held[[0, 4, 6]].any() and x['clock'].tolist() == [40, 40]


# ---------------------------------------------------------------- GR5
def _entry(sim, signals, reservation, n, graph=0, actuation=None, advice=None, **over):
    """mpcx_closed_loop_run_reserved itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, retire=sim._retire, scene=sim._scene)
    st.update(over)
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_reserved(c._ctx, C.byref(cip), C.byref(st['desc']), None, byref(sim._opts), byref(st['retire']),
                                               byref(st['scene']), byref(sim._admit), byref(sim._respawn), byref(sim._routes),
                                               byref(sim._precedence), byref(signals), byref(actuation), byref(advice), None,
                                               byref(reservation), int(n), int(graph)))


def _controllers():
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller
    return [two_phase_controller(10, 40, 5, 8, 12, detect=DETECT), two_phase_controller(6, 25, 3, 5, 9, detect=DETECT)]


def test_off_means_off(ctx, stock):
    """GR5.  After unsignalise() the run equals a batch that never had the rule, bit for bit (40 steps); reservation = NULL and an all-zero
    struct through mpcx_closed_loop_run_reserved give the bytes of the same run through the narrower entry points, without signals and with
    a fixed plan; reserve() after actuate() and actuate() / signalise() after reserve() leave one source of the hold only."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    base = _scene(ctx, stock, reserved=False)
    base.run(40)
    want = base.snapshot()
    sim = _scene(ctx, stock)
    sim.unsignalise()
    assert sim._reservation is None and sim._signals is None
    sim.run(40)
    got = sim.snapshot()
    assert 'held' not in got and 'granted' not in got and 'since' not in got and 'occupied' not in got
    _same(got, want, 'unsignalise')
    assert not sim.granted.any() and (sim.since == -1).all() and not sim.junction_clock.any() and not sim.held.any()     # no longer read or written
    for name, rv in (('NULL', None), ('zero struct', _lib.ReservationC())):
        sim = _scene(ctx, stock, reserved=False)
        _entry(sim, None, rv, 40)
        _same(sim.snapshot(), want, name)
    rsv = _scene(ctx, stock); rsv.run(40)
    r = _snap(rsv)
    assert r['state'].tobytes() != want['state'].tobytes() and r['held'].any() and r['granted'].any()
    # a fixed plan with no reservation: the signals' own run
    plan = two_phase_plan(**G.PLAN)
    fixed = _scene(ctx, stock, reserved=False); fixed.signalise(plan); fixed.run(40)
    want = fixed.snapshot()
    for name, rv in (('NULL', None), ('zero struct', _lib.ReservationC())):
        sim = _scene(ctx, stock, reserved=False); sim.signalise(plan)
        _entry(sim, sim._signals, rv, 40)
        _same(sim.snapshot(), want, 'plan, ' + name)
    sim = _scene(ctx, stock); sim.signalise(plan)               # signalise() after reserve()
    assert sim._reservation is None
    sim.run(40)
    _same(sim.snapshot(), want, 'signalise after reserve')
    act = _scene(ctx, stock, reserved=False); act.actuate(_controllers(), ctrl_of=np.array([0, 1])); act.run(40)
    sim = _scene(ctx, stock); sim.actuate(_controllers(), ctrl_of=np.array([0, 1]))         # actuate() after reserve()
    assert sim._reservation is None and sim._actuation is not None
    sim.run(40)
    _same(sim.snapshot(), act.snapshot(), 'actuate after reserve')
    for first in ('actuate', 'signalise'):                      # reserve() after actuate() / signalise()
        sim = _scene(ctx, stock, reserved=False)
        sim.actuate(_controllers(), ctrl_of=np.array([0, 1])) if first == 'actuate' else sim.signalise(plan)
        sim.reserve(_managers(), manager_of=np.array([0, 1]))
        assert sim._actuation is None and sim._reservation is not None and sim._signals.n_plans == 0
        sim.run(40)
        _same(_snap(sim), r, 'reserve after ' + first)


# ---------------------------------------------------------------- GR6
def test_refusals(ctx, stock):
    """GR6.  MPCX_E_INVALID with a "reservation: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: a NULL pointer, a nonzero reserved word, reservations without signals, with a fixed plan, with actuation, with
    advice, n_per outside 1..64, n_per n_junctions != P, n_mgr < 1, detect < 1, patience < 0, conflict not symmetric, with a diagonal bit or
    with bits at or above n_groups, lane without its own bit, not symmetric or with bits at or above n_groups, the signals' own refusals,
    the agent-sharded layout, more than one linearisation pass; the stage-level call refuses the same way.  In Python: malformed managers
    and tables."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _scene(ctx, stock)
    before = _snap(sim)
    sg, rv = sim._signals, sim._reservation
    names = [n for n, _ in _lib.ReservationC._fields_]
    good = {n: getattr(rv, n) for n in names}
    make = lambda **kw: _lib.ReservationC(**dict(good, **kw))

    def refused(match, reservation, signals=sg, **over):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _entry(sim, signals, reservation, n, graph, **over)
    for n in names[:10]:
        refused(r'mpcx error -1: reservation: %s is null' % n, make(**{n: None}))
    refused(r'mpcx error -1: reservation: a reserved word is not 0', make(reserved=1))
    refused(r'mpcx error -1: reservation: needs signals', rv, signals=None)
    planned = _scene(ctx, stock, reserved=False); planned.signalise(two_phase_plan(**G.PLAN))
    refused(r'mpcx error -1: reservation: the signals also carry a fixed plan', rv, signals=planned._signals)
    act = _scene(ctx, stock, reserved=False); act.actuate(_controllers(), ctrl_of=np.array([0, 1]))
    refused(r'mpcx error -1: reservation: the run also carries actuation', rv, actuation=act._actuation)
    advised = ctx.f64(np.zeros(8)); ctx.synchronize()
    refused(r'mpcx error -1: reservation: the run also carries advice', rv, advice=_lib.AdviceC(advised.data_ptr(), 5.0, 1.0, 60.0, 1, 8))
    sg_names = [n for n, _ in _lib.SignalsC._fields_]
    sgood = {n: getattr(sg, n) for n in sg_names}
    refused(r'mpcx error -1: reservation: signals\.held is null', rv, signals=_lib.SignalsC(**dict(sgood, held=None)))
    refused(r'mpcx error -1: reservation: signals\.n_groups = 17 outside 1\.\.16', rv, signals=_lib.SignalsC(**dict(sgood, n_groups=17)))
    refused(r'mpcx error -1: reservation: signals\.n_points = 0', rv, signals=_lib.SignalsC(**dict(sgood, n_points=0)))
    refused(r'mpcx error -1: reservation: signals\.brake = 0 must be finite and positive', rv, signals=_lib.SignalsC(**dict(sgood, brake=0.0)))
    refused(r'mpcx error -1: reservation: a reserved word is not 0', rv, signals=_lib.SignalsC(**dict(sgood, reserved=2)))
    for n in (0, -2, 65):
        refused(r'mpcx error -1: reservation: n_per = %d outside 1\.\.64' % n, make(n_per=n))
    refused(r'mpcx error -1: reservation: n_per \* n_junctions = 4 \* 3 is not P = 8', make(n_junctions=3))
    refused(r'mpcx error -1: reservation: n_per \* n_junctions = 8 \* 2 is not P = 8', make(n_per=8))
    refused(r'mpcx error -1: reservation: n_mgr = 0', make(n_mgr=0))

    stock_cf = sim._signal_tabs['conflict'].cpu().numpy().astype(np.int64)
    stock_ln = sim._signal_tabs['lane'].cpu().numpy().astype(np.int64)
    assert len(stock_cf) == 12 and stock_cf[1] & (1 << 4) and not stock_cf[1] & (1 << 7)       # straight from the south against from the west / north

    def tables(conflict=None, lane=None, times=((DETECT, 0), (DETECT, 5))):
        cf = stock_cf.copy() if conflict is None else conflict
        ln = stock_ln.copy() if lane is None else lane
        t = (ctx.i32(np.asarray(cf)), ctx.i32(np.asarray(ln)), ctx.i32(np.array(times)))
        ctx.synchronize()
        return t, make(conflict=t[0].data_ptr(), lane=t[1].data_ptr(), mgr_time=t[2].data_ptr(), n_mgr=len(times))
    edit = lambda tab, g, v: np.concatenate([tab[:g], [v], tab[g + 1:]])
    for kw, match in ((dict(conflict=edit(stock_cf, 1, stock_cf[1] & ~(1 << 4))), r'conflict is not symmetric at movements 1 and 4'),
                      (dict(conflict=edit(stock_cf, 3, stock_cf[3] | 8)), r'movement 3 conflicts with itself'),
                      (dict(conflict=edit(stock_cf, 0, stock_cf[0] | 1 << 12)), r'movement 0 has conflict = 0x%x, lane = 0x7 with bits at or above n_groups = 12' % (stock_cf[0] | 1 << 12)),
                      (dict(lane=edit(stock_ln, 5, 0x18)), r'lane\[5\] = 0x18 lacks its own bit'),
                      (dict(lane=edit(stock_ln, 5, 0x38 | 1)), r'lane is not symmetric at movements 0 and 5'),
                      (dict(lane=edit(stock_ln, 11, 0xe00 | 1 << 15)), r'movement 11 has conflict = 0x%x, lane = 0x8e00 with bits at or above' % stock_cf[11]),
                      (dict(times=((0, 0), (DETECT, 5))), r'manager 0 has detect = 0'),
                      (dict(times=((DETECT, 0), (DETECT, -1))), r'manager 1 has patience = -1')):
        keep, bad = tables(**kw)
        refused(r'mpcx error -1: reservation: ' + match, bad)
    keep, fine = tables(times=((1, 0), (1, RH.UNBOUNDED)))      # the limits themselves are accepted
    _entry(sim, sg, fine, 0)
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 2, 4, sim.obs6.data_ptr()
    refused(r'mpcx error -1: reservation: not supported in the agent-sharded layout', rv, desc=shard, retire=None, scene=None)
    ctx.set_linearisation_passes(2)
    try:
        sim.lin_passes = 2
        refused(r'mpcx error -1: reservation: 2 linearisation passes', rv, retire=None, scene=None)
        with pytest.raises(MpcxError, match='reservation: 2 linearisation passes'):
            ctx.reserve_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg, rv)
    finally:
        sim.lin_passes = 1
        ctx.set_linearisation_passes(1)
    # the stage-level call refuses the same way, before its launch
    for bad, match in ((make(grant=None), 'grant is null'), (make(n_per=70), 'n_per = 70'), (make(n_junctions=5), r'is not P = 8'),
                       (tables(times=((-4, 0),))[1], 'detect = -4')):
        with pytest.raises(MpcxError, match='reservation: .*' + match):
            ctx.reserve_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg, bad, done=sim.done)
    with pytest.raises(MpcxError, match='reservation: the signals also carry a fixed plan'):
        ctx.reserve_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], planned._signals, rv)
    ctx.synchronize()
    _same(_snap(sim), before, 'refused')
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # ---- Python
    n = int(sim.path.shape[0])
    mg = _managers()[0]
    for kw in (dict(managers=[]), dict(managers=dict(detect=0, patience=0)), dict(managers=dict(detect=5, patience=-1)),
               dict(managers=mg, stop=np.zeros(n, dtype=np.int32)), dict(managers=mg, stop=np.zeros(3, dtype=np.int32), group=np.zeros(3, dtype=np.int32),
                                                                          exit=np.zeros(3, dtype=np.int32)),
               dict(managers=mg, conflict=np.zeros(12, dtype=np.int32)), dict(managers=mg, conflict=np.zeros(17, dtype=np.int32), lane=np.zeros(17, dtype=np.int32)),
               dict(managers=mg, manager_of=np.zeros(8, dtype=np.int64)), dict(managers=mg, manager_of=np.zeros(2))):
        with pytest.raises(ValueError):
            sim.reserve(**kw)
    assert sim._reservation is rv and sim._signals is sg
    sim.unsignalise()
    assert sim._reservation is None and sim._signals is None and 'granted' not in sim.snapshot()
