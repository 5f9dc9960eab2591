"""GPU tests of the PRIORITY ROAD in the device-resident closed loop (mpcx_set_priority, mpcx_priority_step_batch,
IntersectionBatch.priority_road): priority_kernel runs in the hold's place -- a lane group per junction classifies the junction's agents,
every lane meets every other lane of its group by rotating shuffles and keeps the least time to the line among the conflicting agents of
smaller rank, and an agent whose lag is below its critical gap is held at its stop line.  The stage call against the host build of the rule
on the hand-made junctions of tests/test_priority_cpu.py and on random words at every lane-group size; the two scenes of
tests/priority_helpers.py in the closed loop against the oracle loop; graph replay, host staging, off means off, the refusals, a struct
changed under graph replay.  T = 13, v0 = 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import keepclear_helpers as KH
from tests import priority_helpers as PH
from tests import test_gpu_respawn as GR

pytestmark = pytest.mark.gpu

TOL = 2e-7                              # the bar of every closed-loop replay here
OWN = ('yielding', 'yield_waited', 'blocker', 'lag', 'crossing', 'n_yielding')


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
    return PH.build_ref(tmp_path_factory.mktemp('priority_ref'))


def _scene(c, stock, name='two', mode='cut', rule=True, retire=True, **kw):
    """a scene of priority_helpers as a batch of one instance"""
    sim = GR._batch(c, stock, np.array(PH.SCENE_ROUTES[name]), np.array([PH.SCENES[name][1]]), mode)
    if not retire:
        sim.keep_driving()
    if rule:
        sim.priority_road(gap=PH.GAP_S, v_floor=PH.V_FLOOR_S, **kw)
    return sim


def _same(a, b, what, skip=()):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in b:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---------------------------------------------------------------- GP1
def _device_stage(c, w):
    """mpcx_priority_step_batch on the words of priority_helpers.words(); returns OUT_KEYS as the device left them"""
    from mpc_for_av_at_intersection_amd import _lib
    d = {k: c.i32(w[k]) for k in PH.I32_KEYS}
    d.update({k: c.f64(w[k]) for k in PH.F64_KEYS})
    done = None if w['done'] is None else c.i32(w['done'])
    pr = _lib.PriorityC(d['path_stop'].data_ptr(), d['path_move'].data_ptr(), d['path_exit'].data_ptr(), d['conflict'].data_ptr(),
                        d['rank'].data_ptr(), d['gap'].data_ptr(), d['waited'].data_ptr(), d['yielding'].data_ptr(), d['blocker'].data_ptr(),
                        d['lag'].data_ptr(), d['occupied'].data_ptr(), d['n_yielding'].data_ptr(), float(w['v_floor']), float(w['brake']),
                        int(w['detect']), int(w['n_per']), len(w['occupied']), len(w['conflict']), len(w['path_stop']), 0)
    c.synchronize()
    c.priority_step(float(w['dl']), d['state'], d['path_off'], d['path_len'], d['traj_idx'], d['cut_len'], pr, done=done)
    c.synchronize()
    got = {k: d[k].cpu().numpy() for k in PH.I32_KEYS + PH.F64_KEYS}
    for k in got:               # nothing but the outputs is written
        if k not in PH.OUT_KEYS:
            assert got[k].tobytes() == w[k].tobytes(), k
    if done is not None:
        assert done.cpu().numpy().tobytes() == w['done'].tobytes()
    return {k: got[k] for k in PH.OUT_KEYS}


@pytest.mark.parametrize('n_per,J', [(1, None), (3, None), (8, None), (64, None), (8, 1), (8, 33)], ids=lambda v: 'all' if v is None else str(v))
def test_stage_call_equals_the_host_build(ctx, ref, n_per, J):
    """GP1.  mpcx_priority_step_batch equals the host build byte for byte on every in-out and out word -- cut_len, waited, yielding,
    blocker, lag, occupied, n_yielding -- and the values written down by hand, with and without the retirement words, on the hand-made
    junctions and on seeded random words: n_per = 1 (a lane per junction, no shuffle), 3 (a padding lane in every group of 4), 8, 64 (a
    wavefront per junction); one junction alone; 33 junctions of 8 = five wavefronts, the last with one live group of eight."""
    w, want = PH.hand_made(n_per, repeat=2 if J == 33 else 1)
    if J == 1:
        j0 = next(i for i, c in enumerate(PH.CASES) if c[0].startswith('three ranks'))
        w = PH.junctions(w, j0, j0 + 1)
    elif J is not None:
        w = PH.junctions(w, 0, J)
    assert J is None or len(w['occupied']) == J
    cases = [(w, True), (w, False)] + [(PH.random_words(seed, n_per, len(w['occupied'])), True) for seed in (1, 2)]
    for k, (case, with_done) in enumerate(cases):
        host = PH.copy_words(case)
        if not with_done:
            host['done'] = None
        got = _device_stage(ctx, host)
        n = PH.host_rule(ref, host)
        for key in PH.OUT_KEYS:
            assert got[key].tobytes() == host[key].tobytes(), (key, k, np.flatnonzero(got[key] != host[key]))
        assert n == int(got['yielding'].sum()) == int(got['n_yielding'].sum())
        if k == 0 and J is None:
            PH.check_against_want(dict(got), want, w)
        if k == 0 and J == 1:
            assert got['n_yielding'].tolist() == [2] and got['occupied'].tolist() == [0]
            assert sorted(got['lag'].tolist())[:2] == [0.5, 2.0] and sorted(got['blocker'].tolist())[-2:] == [0, 4]    # (slots 0, 4, 7 of eight)


# ---------------------------------------------------------------- GP2
def _sync(loop, before, rows):
    """the oracle loop's continuous words from the device's before the step (the integers -- waited among them -- run on their own)"""
    loop.state, loop.applied = before['state'][rows].copy(), before['applied'][rows].copy()
    loop.traj_idx, loop.target = [int(v) for v in before['traj_idx'][rows]], [int(v) for v in before['target_ind'][rows]]
    loop.prev = [int(v) for v in before['prev_cut'][rows]]
    loop.u = [before['u'][p].copy() for p in rows]


def _device_entries(loop, before, after):
    """the short-gap entries of a step from the device's own words: the state before the step, traj_idx as the step left it"""
    drive = [not d for d in before['done']]
    w = PH.words(state=before['state'], traj_idx=after['traj_idx'], cut_len=after['cut_len'], done=[0 if d else 1 for d in drive],
                 waited=np.zeros(loop.A), yielding=np.zeros(loop.A), blocker=np.zeros(loop.A), lag=np.zeros(loop.A), occupied=[0], n_yielding=[0],
                 **loop.tab)
    kinds = [KH.classify(w, q) for q in range(loop.A)]
    return PH.short_gap_entries(w, kinds, [int(v) for v in before['traj_idx']], drive)


def _replay(sim, loop, n_steps):
    """n_steps of `sim` (one instance; or fewer, once everybody has arrived), every one replayed on `loop` from the device's own state
    before the step; returns (worst |GPU - oracle|, yielding steps per agent, arrival steps, short-gap entries on the device)"""
    rows = list(range(sim.P))
    worst, yield_steps, arr, entries = 0.0, np.zeros(sim.P, dtype=np.int64), np.full(sim.P, -1), []
    on = sim._priority is not None
    for s in range(n_steps):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        assert [bool(d) for d in before['done']] == loop.done and [bool(d) for d in before['absent']] == loop.absent, s
        _sync(loop, before, rows)
        out = loop.step()
        if on:
            for k, v in (('yielding', loop.yielding), ('yield_waited', loop.waited), ('blocker', loop.blocker)):
                assert after[k].tolist() == v.tolist(), (s, k, after[k], v)
            assert after['lag'].tobytes() == np.asarray(loop.lag, np.float64).tobytes(), (s, after['lag'], loop.lag)
            assert int(after['crossing'][0]) == loop.occ_hist[-1] and int(after['n_yielding'][0]) == loop.n_yielding, (s, after['crossing'])
            yield_steps += after['yielding'] != 0
        else:
            assert not any(k in after for k in OWN)
        for a in rows:
            r = out[a]
            if r is None:
                assert before['done'][a] and (not on or (after['yielding'][a] == 0 and after['yield_waited'][a] == 0 and after['blocker'][a] == -1))
                continue
            want = (r['traj_idx'], r['cut'], r['target'], r['hit'], r['status'])
            got = (after['traj_idx'][a], after['cut_len'][a], after['target_ind'][a], after['hit_idx'][a], after['status'][a])
            assert want == tuple(int(v) for v in got), (s, a, want, got)
            worst = max(worst, float(np.abs(r['u_sol'] - after['u'][a]).max()), float(np.abs(r['x_sol'] - after['x'][a]).max()),
                        float(np.abs(r['post'] - after['state'][a]).max()))
            assert bool(after['done'][a]) == loop.done[a], (s, a)
        entries += [(s,) + e for e in _device_entries(loop, before, after)]
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        if after['done'].all():
            break
    assert [e[:3] for e in entries] == [e[:3] for e in loop.entries]
    return worst, yield_steps, arr, entries


@pytest.mark.parametrize('name,mode', [('two', 'cut'), ('four', 'cut'), ('two', 'speed')])
def test_scenes_on_the_oracle(ctx, stock, name, mode):
    """GP2.  The scenes of tests/test_priority_cpu.py P4 in the device loop, rule on and off, until everybody has arrived, every step
    replayed on a PriorityLoop from the device's own state before the step (the loop's integers are never re-synchronised).  traj_idx,
    cut_len, target index, hit, status, yielding, yield_waited, blocker, crossing and n_yielding are identical, lag bit for bit; states and
    solutions agree within 2e-7; the arrivals are the oracle's.  In cut mode, with the rule there is no short-gap entry as computed from
    the device's own words, the rank-0 car never yields and the others do; THE SAME RUN WITH THE STAGE OFF HAS SUCH AN ENTRY -- the
    assertion that fails without the feature.  Speed mode (two cars): parity only."""
    speed = mode == 'speed'
    res = {}
    for on in (True, False):
        sim = _scene(ctx, stock, name, mode, rule=on)
        loop = PH.scene_loop(name, on, speed=speed)
        if on:
            assert sim._priority.detect == loop.tab['detect'] and sim._priority.brake == loop.tab['brake'] and sim.dl == loop.dl
            assert np.array_equal(sim._priority_tabs['rank'].cpu().numpy(), loop.tab['rank'])
            cf = sim._priority_tabs['conflict'].cpu().numpy()
            assert all((int(cf[g]) >> h) & 1 == (int(loop.tab['conflict'][g]) >> h) & 1 for g in loop.movement for h in loop.movement)
        worst, yield_steps, arr, entries = _replay(sim, loop, PH.STEPS)
        print('%s cars, %s, rule %s: worst |GPU - oracle| %.2e, arrivals %s, yielding steps %s, entries %s'
              % (name, mode, on, worst, arr.tolist(), yield_steps.tolist(), entries))
        assert worst < TOL, worst
        assert (arr > 0).all() and arr.tolist() == loop.arrival
        res[on] = (yield_steps, entries, loop)
    assert res[True][0][0] == 0 and res[True][0][1:].sum() >= 1 and not res[False][0].any()
    if not speed:
        assert res[True][1] == [] and len(res[False][1]) >= 1
        assert (res[True][0][1:] >= 1).all()
        assert not any(c[5] == 'exempt' for c in res[True][2].candidates)
        assert res[True][2].worst_clearance > 0.0 and res[True][2].worst_clearance >= res[False][2].worst_clearance


# ---------------------------------------------------------------- GP3
@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    from tests import stack_helpers as K
    return K.build_libs(tmp_path_factory.mktemp('priority_stack_ref'))


def _flow(c, stock):
    """the lifecycle scene of priority_helpers: one instance of eight slots, admission, respawn with routes, give_way('entry'), the
    priority rule, following"""
    routes, dl, cd = stock
    sc, tab = PH.flow_scene(routes)
    sim = GR._batch(c, stock, sc['route_of'][:, :, 0], sc['start_idx'][:, :, 0], 'cut')      # (retire_at_goal(leave_scene=True))
    sim.respawn_on_schedule(sc['due'], gap=sc['gap'], route=sc['route_of'], start_index=sc['start_idx'])
    sim.give_way('entry')
    sim.priority_road(gap=PH.GAP_S, v_floor=PH.V_FLOOR_S)
    sim.follow(**sc['follow'])
    return sim, tab


def _flow_snap(sim):
    """snapshot() and the device words it leaves out, under the names of stack_helpers"""
    out = sim.snapshot()
    get = lambda t: t.cpu().numpy().copy()
    out.update(path_off=get(sim.path_off), path_len=get(sim.path_len), clock=get(sim.clock), ep_i32=get(sim.ep_i32), ep_f64=get(sim.ep_f64))
    return out


def test_lifecycle(ctx, stock, libs):
    """GP3.  The priority rule beside following, give_way('entry'), retirement with leave_scene=True and respawn with routes: one
    instance of eight slots (stack_helpers' scene without its lights), 150 steps, every one before = snapshot, run(1), after = snapshot
    with `after` = priority_helpers.flow_step(before).  Integer words identical -- yielding, yield_waited, blocker, crossing, n_yielding
    among them --, gap, follow_cap and lag bit for bit, u, x, state and applied within 2e-7.  The run has yielding cars in every
    minor-road slot, candidates that waited and candidates that could stop, slots reset and served again with their waited word healed,
    and no short-gap entry (tests/test_priority_cpu.py shows the same on the host composition alone)."""
    from tests import stack_helpers as K
    sim, tab = _flow(ctx, stock)
    cfg, first = PH.flow_config(libs, K.stock_paths()[0], K.stock_paths()[1])
    assert np.array_equal(sim.path.cpu().numpy(), cfg.path) and sim.dl == cfg.dl
    for k in ('path_stop', 'path_move', 'path_exit', 'conflict', 'rank', 'gap'):
        assert np.array_equal(sim._priority_tabs[k].cpu().numpy(), cfg.priority[k]), k
    assert sim._priority.detect == cfg.priority['detect'] and sim._priority.brake == cfg.priority['brake'] and sim._priority.v_floor == cfg.priority['v_floor']
    before = _flow_snap(sim)
    for k in K.INT_WORDS + PH.FLOW_INT + ('lag',):
        if k in first and k in before:
            assert np.array_equal(first[k], before[k]), k
    worst, yield_steps, why, entries, healed = 0.0, np.zeros(cfg.P, np.int64), {}, [], 0
    for s in range(PH.FLOW_STEPS):
        sim.run(1)
        after = _flow_snap(sim)
        want, info = PH.flow_step(cfg, before)
        worst = max(worst, K.compare_words(after, want, cfg, what=s))
        for k in PH.FLOW_INT:
            assert np.array_equal(after[k], want[k]), (s, k, after[k], want[k])
        assert after['lag'].tobytes() == want['lag'].tobytes(), (s, after['lag'], want['lag'])
        yield_steps += after['yielding'] != 0
        for c in info['candidates']:
            why[c[5]] = why.get(c[5], 0) + 1
        entries += [(s,) + e for e in info['entries']]
        healed += sum(1 for q in info['admitted'] if before['served'][q] > 0 and not before['yield_waited'][q])
        before = after
    sim.check()
    print('lifecycle: worst |GPU - oracle| %.2e, yielding steps %s, candidates %s, served %s' % (worst, yield_steps.tolist(), why, before['served'].tolist()))
    assert entries == [] and all(yield_steps[q] >= 1 for q in PH.FLOW_MINOR) and why.get('waited', 0) > 0 and why.get('can stop', 0) > 0
    assert before['served'].sum() >= cfg.P and healed >= 1


# ---------------------------------------------------------------- GP4
def test_graph_replay_and_host_staging(ctx, stock):
    """GP4.  8 chunks of run(5, graph=True) on a side stream equal 40 x run(1) plain, byte for byte, the stage's six buffers included;
    step_staged() -- the per-stage entry points with mpcx_priority_step_batch in the hold's place -- equals run(1) after every one of 40
    steps on the loop without retirement.  The 40 steps span the minor car's free approach and its wait at the line."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _scene(ctx, stock)
    seen = set()
    for _ in range(40):
        plain.run(1)
        seen.add(int(plain.n_yielding[0]))
    a = plain.snapshot()
    assert seen == {0, 1} and all(k in a for k in OWN)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _scene(side, stock)
        torch.cuda.synchronize()
        for _ in range(8):
            graph.run(5, graph=True)
        _same(graph.snapshot(), a, 'graph')
    finally:
        side.close()
    X, Y = (_scene(ctx, stock, retire=False) for _ in range(2))
    yielding = 0
    for s in range(40):
        X.run(1); Y.step_staged()
        x = X.snapshot()
        _same(Y.snapshot(), x, s)
        yielding += int(x['yielding'][1])
    assert yielding >= 10 and not x['yielding'][0]


# ---------------------------------------------------------------- GP5
def test_off_means_off(ctx, stock):
    """GP5.  priority_road() then all_roads_equal() gives the bytes of a batch that never had the stage: every buffer of snapshot(), sol
    and the run log (45 steps: past the entry the stage would have prevented).  With an all-zero conflict table, or with gap = 0, the
    stage is on and writes its own words only, and everything else equals the plain run.  A run with the stage really on differs.
    signalise(), actuate() and reserve() switch the stage off."""
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller, two_phase_plan
    base = _scene(ctx, stock, rule=False)
    base.attach_log(45)
    base.run(45)
    want, rows = base.snapshot(), base.log.rows()
    sim = _scene(ctx, stock)
    sim.all_roads_equal()
    assert sim._priority is None
    sim.attach_log(45)
    sim.run(45)
    got = sim.snapshot()
    assert not any(k in got for k in OWN)
    _same(got, want, 'all_roads_equal')
    assert sim.log.rows().tobytes() == rows.tobytes()
    assert all(sim.sol[k].cpu().numpy().tobytes() == v.cpu().numpy().tobytes() for k, v in base.sol.items() if torch.is_tensor(v))
    assert not sim.yielding.any() and not sim.yield_waited.any() and not sim.crossing.any() and (sim.blocker == -1).all()      # no longer written
    for what, kw in (('zero table', dict(conflict=np.zeros(12, dtype=np.int32))), ('gap 0', dict(gap=0.0))):
        zero = _scene(ctx, stock, rule=False)
        zero.priority_road(**dict(dict(gap=PH.GAP_S), **kw))
        zero.attach_log(45)
        seen, lags = set(), 0
        for _ in range(45):
            zero.run(1)
            seen.add(int(zero.crossing[0]))
            lags += int(torch.isfinite(zero.lag).sum())
        got = zero.snapshot()
        assert all(k in got for k in OWN) and not got['yielding'].any() and not got['yield_waited'].any() and {0, 1 << 4} <= seen, (what, seen)
        assert (lags > 0) == (what == 'gap 0')          # (gap = 0: the lag is written, nobody is threatened)
        _same({k: v for k, v in got.items() if k not in OWN}, want, what)
        assert zero.log.rows().tobytes() == rows.tobytes()
    on = _scene(ctx, stock); on.run(45)
    assert on.snapshot()['state'].tobytes() != want['state'].tobytes()
    for switch in (lambda s: s.signalise(two_phase_plan(cycle=100, green=30, amber=8)),
                   lambda s: s.actuate(two_phase_controller(detect=144, min_green=5, max_green=40, gap=2, amber=2, all_red=0)),
                   lambda s: s.reserve(dict(detect=144, patience=0))):
        sim = _scene(ctx, stock)
        switch(sim)
        assert sim._priority is None and sim._signals is not None and 'yielding' not in sim.snapshot()
        sim.run(2)
        with pytest.raises(ValueError, match='priority_road: the batch runs under'):
            sim.priority_road()


# ---------------------------------------------------------------- GP6
def _run_entry(sim, n, graph=0, signals=None, actuation=None, reservation=None, **over):
    """the widest entry point itself with the structs of `sim` unless given (the stage is the context's: _claim_context sets it)"""
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, retire=sim._retire, scene=sim._scene)
    st.update(over)
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_reserved(c._ctx, C.byref(cip), C.byref(st['desc']), None, byref(sim._opts), byref(st['retire']),
                                               byref(st['scene']), byref(sim._admit), byref(sim._respawn), byref(sim._routes),
                                               byref(sim._precedence), byref(signals), byref(actuation), None, None, byref(reservation),
                                               int(n), int(graph)))


def test_refusals(ctx, stock):
    """GP6.  MPCX_E_INVALID with a "priority: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: a NULL pointer among the twelve, n_per outside 1..64, n_per n_junctions != P, n_moves outside 1..16, n_points <
    1, detect < 1, v_floor or brake not finite or not positive, a nonzero reserved word, signals, actuation or a reservation in the run,
    the agent-sharded layout, more than one linearisation pass, a conflict word with bits at or above n_moves, with its own bit or
    asymmetric, a negative rank, a gap that is negative or not finite; the stage-level call refuses the same way.  In Python:
    priority_road() under signals, with malformed tables, with more than 64 agents per junction."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _scene(ctx, stock)
    before = sim.snapshot()
    pr = sim._priority
    names = [n for n, _ in _lib.PriorityC._fields_]
    good = {n: getattr(pr, n) for n in names}
    make = lambda **kw: _lib.PriorityC(**dict(good, **kw))
    keep = []

    def refused(match, struct, **over):
        for graph in (0, 1):
            for n in (0, 1):
                sim._claim_context()
                ctx.set_priority(struct)
                try:
                    with pytest.raises(MpcxError, match=match):
                        _run_entry(sim, n, graph, **over)
                finally:
                    ctx.set_priority(None)
    for n in names[:12]:
        refused(r'mpcx error -1: priority: %s is null' % n, make(**{n: None}))
    refused(r'mpcx error -1: priority: the reserved word is not 0', make(reserved=1))
    lit = _scene(ctx, stock, rule=False); lit.signalise(two_phase_plan(cycle=100, green=30, amber=8))
    act = _scene(ctx, stock, rule=False); act.actuate(two_phase_controller(detect=144, min_green=5, max_green=40, gap=2, amber=2, all_red=0))
    rsv = _scene(ctx, stock, rule=False); rsv.reserve(dict(detect=144, patience=0))
    held = r'mpcx error -1: priority: the run also carries signals, actuation or a reservation'
    refused(held, pr, signals=lit._signals)
    refused(held, pr, signals=act._signals, actuation=act._actuation)
    refused(held, pr, signals=rsv._signals, reservation=rsv._reservation)
    for n in (0, -2, 65):
        refused(r'mpcx error -1: priority: n_per = %d outside 1\.\.64' % n, make(n_per=n))
    refused(r'mpcx error -1: priority: n_per \* n_junctions = 2 \* 3 is not P = 2', make(n_junctions=3))
    refused(r'mpcx error -1: priority: n_per \* n_junctions = 1 \* 1 is not P = 2', make(n_per=1))
    for n in (0, 17):
        refused(r'mpcx error -1: priority: n_moves = %d outside 1\.\.16' % n, make(n_moves=n))
    for n in (0, -5):
        refused(r'mpcx error -1: priority: n_points = %d' % n, make(n_points=n))
    for d in (0, -3):
        refused(r'mpcx error -1: priority: detect = %d' % d, make(detect=d))
    for v in (0.0, -1.0, float('nan'), float('inf')):
        refused(r'mpcx error -1: priority: v_floor = ', make(v_floor=v))
        refused(r'mpcx error -1: priority: brake = ', make(brake=v))
    stock_cf = sim._priority_tabs['conflict'].cpu().numpy().astype(np.int64)
    stock_rk = sim._priority_tabs['rank'].cpu().numpy()
    stock_gp = sim._priority_tabs['gap'].cpu().numpy()
    assert len(stock_cf) == 12 and stock_cf[1] & (1 << 4) and not stock_cf[1] & (1 << 7)       # straight from arm 1 against from arm 2 / arm 3

    def table(name, v, **kw):
        t = ctx.f64(np.asarray(v, np.float64)) if name == 'gap' else ctx.i32(np.asarray(v))
        ctx.synchronize()
        keep.append(t)
        return make(**dict({name: t.data_ptr()}, **kw))
    edit = lambda tab, g, v: np.concatenate([tab[:g], [v], tab[g + 1:]])
    refused(r'mpcx error -1: priority: conflict is not symmetric at movements 1 and 4', table('conflict', edit(stock_cf, 1, stock_cf[1] & ~(1 << 4))))
    refused(r'mpcx error -1: priority: movement 3 conflicts with itself', table('conflict', edit(stock_cf, 3, stock_cf[3] | 8)))
    refused(r'mpcx error -1: priority: movement 0 has conflict = 0x%x with bits at or above n_moves = 12' % (stock_cf[0] | 1 << 12),
            table('conflict', edit(stock_cf, 0, stock_cf[0] | 1 << 12)))
    refused(r'mpcx error -1: priority: movement \d+ has conflict = 0x[0-9a-f]+ with bits at or above n_moves = 4', table('conflict', stock_cf, n_moves=4))
    refused(r'mpcx error -1: priority: movement 5 has the negative rank -1', table('rank', edit(stock_rk, 5, -1)))
    refused(r'mpcx error -1: priority: movement 2 has gap = -0\.5', table('gap', edit(stock_gp, 2, -0.5)))
    refused(r'mpcx error -1: priority: movement 11 has gap = inf', table('gap', edit(stock_gp, 11, np.inf)))
    refused(r'mpcx error -1: priority: movement 0 has gap = nan', table('gap', edit(stock_gp, 0, np.nan)))
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 1, 2, sim.obs6.data_ptr()
    refused(r'mpcx error -1: priority: not supported in the agent-sharded layout', pr, desc=shard, retire=None, scene=None)
    args = (sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'])
    ctx.set_linearisation_passes(2)
    try:
        sim.lin_passes = 2
        refused(r'mpcx error -1: priority: 2 linearisation passes', pr, retire=None, scene=None)
        with pytest.raises(MpcxError, match='priority: 2 linearisation passes'):
            ctx.priority_step(*args, pr)
    finally:
        sim.lin_passes = 1
        ctx.set_linearisation_passes(1)
    # the stage-level call refuses the same way, before its launch
    for bad, match in ((make(lag=None), 'lag is null'), (make(n_per=70), 'n_per = 70'), (make(n_junctions=5), r'is not P = 2'), (make(detect=0), 'detect = 0'),
                       (make(reserved=3), 'reserved word'), (make(v_floor=0.0), 'v_floor = 0'), (table('conflict', edit(stock_cf, 3, stock_cf[3] | 8)), 'conflicts with itself'),
                       (table('rank', edit(stock_rk, 0, -4)), 'negative rank -4'), (table('gap', edit(stock_gp, 1, -1.0)), 'gap = -1')):
        with pytest.raises(MpcxError, match='priority: .*' + match):
            ctx.priority_step(*args, bad, done=sim.done)
    ctx.synchronize()
    _same(sim.snapshot(), before, 'refused')
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # the limits themselves are accepted
    ctx.set_priority(make(detect=1)); _run_entry(sim, 0); ctx.set_priority(None)
    # ---- Python
    n = int(sim.path.shape[0])
    for kw in (dict(move=np.zeros(n, dtype=np.int32)), dict(stop=np.zeros(3, dtype=np.int32), move=np.zeros(3, dtype=np.int32), exit=np.zeros(3, dtype=np.int32)),
               dict(conflict=np.zeros(17, dtype=np.int32)), dict(conflict=np.zeros((2, 6), dtype=np.int32)), dict(conflict=np.zeros(12)), dict(detect=0),
               dict(rank=np.zeros(11, dtype=np.int32)), dict(rank=-np.ones(12, dtype=np.int32)), dict(rank=np.zeros(12)), dict(gap=-1.0),
               dict(gap=np.ones(5)), dict(gap=float('nan')), dict(v_floor=0.0), dict(brake=-2.0), dict(major=(7,))):
        with pytest.raises(ValueError):
            sim.priority_road(**kw)
    assert sim._priority is pr
    for other in (lit, act, rsv):
        with pytest.raises(ValueError, match='priority_road: the batch runs under'):
            other.priority_road()
    wide = GR._batch(ctx, stock, np.ones((1, 65), dtype=np.int64), np.zeros((1, 65), dtype=np.int64), 'cut')
    with pytest.raises(ValueError, match='a junction holds 1 .. 64 agents'):
        wide.priority_road()
    sim.all_roads_equal()
    assert sim._priority is None and 'yielding' not in sim.snapshot()


# ---------------------------------------------------------------- GP7
def test_changed_struct_under_graph_replay(stock):
    """GP7.  The cached graph's key covers the struct by value.  Another detect: 10 steps replayed with the whole approach as the detector,
    then detect changed in place to 5 points and 35 more replayed.  Another gap table pointer: 10 steps, then an all-zero table at another
    address, 35 more.  Both equal the same sequence run plain, byte for byte -- and differ from the run under the first struct."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        for change in ('detect', 'gap'):
            sims = [_scene(side, stock) for _ in range(3)]
            torch.cuda.synchronize()
            tabs = []
            for sim, graph, changed in zip(sims, (True, False, True), (True, True, False)):
                sim.run(10, graph=graph)
                if changed and change == 'detect':
                    sim._priority.detect = 5
                elif changed:
                    tabs.append(side.f64(np.zeros(12)))
                    side.synchronize()
                    sim._priority.gap = tabs[-1].data_ptr()
                for _ in range(7):
                    sim.run(5, graph=graph)
            a, b, c = (sim.snapshot() for sim in sims)
            _same(a, b, 'changed ' + change)
            assert a['state'].tobytes() != c['state'].tobytes(), change
    finally:
        side.close()
