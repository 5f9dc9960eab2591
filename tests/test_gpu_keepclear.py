"""GPU tests of KEEP CLEAR in the device-resident closed loop (mpcx_set_keepclear, mpcx_keepclear_step_batch, IntersectionBatch.keep_clear):
keepclear_kernel runs directly behind signal_kernel / actuated_signal_kernel -- a lane group per junction classifies the junction's agents,
ORs the movements inside the crossing by one butterfly and holds an agent whose light lets it go but whose movement conflicts with one that
is inside.  The stage call against the host build of the rule on the hand-made junctions of tests/test_keepclear_cpu.py and on random
words at every lane-group size; the late-straight scene in the closed loop against the oracle loops of tests/keepclear_helpers.py under a
fixed plan (both stop modes) and under a controller; the lifecycle scene (admission, respawn, right of way, following) under a controller;
graph replay, host staging, off means off, the refusals, a struct changed under graph replay.  T = 13, v0 = 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import keepclear_helpers as KH
from tests import test_gpu_respawn as GR

pytestmark = pytest.mark.gpu

LATE_ROUTES = np.array([[1, 3]])        # stock routes (1, 2) and (2, 2): the straights from arms 1 and 2
TOL = 2e-7                              # the bar of tests/test_gpu_reserve.py's oracle tests (and of every closed-loop replay)


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
    return KH.build_ref(tmp_path_factory.mktemp('keepclear_ref'))


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    from tests import stack_helpers as K
    return K.build_libs(tmp_path_factory.mktemp('keepclear_stack_ref'))


def _controller():
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller
    return two_phase_controller(detect=144, **KH.LATE_CONTROLLER)


def _late(c, stock, mode='cut', keep_clear=True, actuated=False, retire=True):
    """the late-straight scene of keepclear_helpers as a batch of one instance: under LATE_PLAN, or under LATE_CONTROLLER"""
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    speed = mode == 'speed'
    sim = GR._batch(c, stock, LATE_ROUTES, np.array([KH.LATE_START[speed]]), mode)
    if not retire:
        sim.keep_driving()
    if actuated:
        sim.actuate(_controller())
    else:
        sim.signalise(two_phase_plan(**KH.LATE_PLAN), offset=np.array([KH.LATE_TICK[speed]]))
    if keep_clear:
        sim.keep_clear()
    return sim


def _snap(sim):
    out = sim.snapshot()
    if sim._actuation is not None:
        out['jstate'], out['calls'] = sim.junction_state.cpu().numpy().copy(), sim.calls.cpu().numpy().copy()
    elif sim._signals is not None:
        out['tick'] = sim.tick.cpu().numpy().copy()
    return out


def _same(a, b, what, skip=()):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in b:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---------------------------------------------------------------- GK1
def _device_stage(c, w):
    """mpcx_keepclear_step_batch on the words of keepclear_helpers.words(); returns OUT_KEYS as the device left them"""
    from mpc_for_av_at_intersection_amd import _lib
    d = {k: c.i32(w[k]) for k in KH.I32_KEYS}
    state = c.f64(w['state'])
    done = None if w['done'] is None else c.i32(w['done'])
    sg = _lib.SignalsC(d['path_stop'].data_ptr(), None, None, None, None, None, None, d['held'].data_ptr(), float(w['brake']), len(w['path_stop']), 0, 1, 0)
    kc = _lib.KeepClearC(d['path_move'].data_ptr(), d['path_exit'].data_ptr(), d['conflict'].data_ptr(), d['boxed'].data_ptr(), d['waited'].data_ptr(),
                         d['occupied'].data_ptr(), d['n_boxed'].data_ptr(), int(w['detect']), int(w['n_per']), len(w['occupied']), len(w['conflict']),
                         len(w['path_stop']), 0)
    c.synchronize()
    c.keepclear_step(float(w['dl']), state, d['path_off'], d['path_len'], d['traj_idx'], d['cut_len'], sg, kc, done=done)
    c.synchronize()
    got = {k: d[k].cpu().numpy() for k in KH.I32_KEYS}
    for k in KH.I32_KEYS:       # nothing but the outputs is written (held among them: it stays the signal stage's)
        if k not in KH.OUT_KEYS:
            assert got[k].tobytes() == w[k].tobytes(), k
    assert state.cpu().numpy().tobytes() == w['state'].tobytes()
    return {k: got[k] for k in KH.OUT_KEYS}


@pytest.mark.parametrize('n_per,J', [(1, None), (3, None), (8, None), (64, None), (8, 1), (8, 33)], ids=lambda v: 'all' if v is None else str(v))
def test_stage_call_equals_the_host_build(ctx, ref, n_per, J):
    """GK1.  mpcx_keepclear_step_batch equals the host build byte for byte on every in-out and out word -- cut_len, boxed, waited, occupied,
    n_boxed -- and the values written down by hand, with and without the retirement words, on the hand-made junctions and on seeded random
    words: n_per = 1 (a lane per junction, no shuffle), 3 (a padding lane in every group of 4), 8, 64 (a wavefront per junction); one
    junction alone; 33 junctions of 8 = five wavefronts, the last with one live group of eight."""
    w, want = KH.hand_made(n_per, repeat=2 if J == 33 else 1)
    if J == 1:
        j0 = next(i for i, c in enumerate(KH.CASES) if c[0].startswith('two movements inside'))
        w = KH.junctions(w, j0, j0 + 1)
    elif J is not None:
        w = KH.junctions(w, 0, J)
    assert J is None or len(w['occupied']) == J
    cases = [(w, True), (w, False)] + [(KH.random_words(seed, n_per, len(w['occupied'])), True) for seed in (1, 2)]
    for k, (case, with_done) in enumerate(cases):
        host = KH.copy_words(case)
        if not with_done:
            host['done'] = None
        got = _device_stage(ctx, host)
        n = KH.host_rule(ref, host)
        for key in KH.OUT_KEYS:
            assert got[key].tobytes() == host[key].tobytes(), (key, k, np.flatnonzero(got[key] != host[key]))
        assert n == int(got['boxed'].sum()) == int(got['n_boxed'].sum())
        if k == 0 and J is None:
            KH.check_against_want(dict(got), want, w)
        if k == 0 and J == 1:
            assert got['n_boxed'].tolist() == [1] and got['occupied'].tolist() == [12]


# ---------------------------------------------------------------- GK2, GK3
def _sync(loop, before, rows):
    """the oracle loop's continuous words from the device's before the step (the integers -- held, boxed, waited, the clock or the
    junction state -- run on their own)"""
    loop.state, loop.applied = before['state'][rows].copy(), before['applied'][rows].copy()
    loop.traj_idx, loop.target = [int(v) for v in before['traj_idx'][rows]], [int(v) for v in before['target_ind'][rows]]
    loop.prev = [int(v) for v in before['prev_cut'][rows]]
    loop.u = [before['u'][p].copy() for p in rows]


def _replay(sim, loop, n_steps):
    """n_steps of `sim` (one instance; or fewer, once everybody has arrived), every one replayed on `loop` from the device's own state
    before the step; returns (worst |GPU - oracle|, boxed steps per agent, arrival steps, entries into an occupied box on the device)"""
    rows = list(range(sim.P))
    worst, boxed_steps, arr, entries = 0.0, np.zeros(sim.P, dtype=np.int64), np.full(sim.P, -1), []
    on = sim._keepclear is not None
    for s in range(n_steps):
        before = _snap(sim)
        sim.run(1)
        after = _snap(sim)
        assert [bool(d) for d in before['done']] == loop.done and [bool(d) for d in before['absent']] == loop.absent, s
        _sync(loop, before, rows)
        out = loop.step()
        assert after['held'].tolist() == loop.held, (s, after['held'], loop.held)
        if on:
            assert after['boxed'].tolist() == loop.boxed.tolist() and after['box_waited'].tolist() == loop.waited.tolist(), (s, after['boxed'], loop.boxed)
            assert int(after['box_occupied'][0]) == loop.occ_hist[-1] and int(after['n_boxed'][0]) == int(loop.boxed.sum()), (s, after['box_occupied'])
            boxed_steps += after['boxed'] != 0
        if sim._actuation is not None:
            assert tuple(after['jstate'][0]) == tuple(loop.jstate) and int(after['calls'][0]) == loop.calls_hist[-1], s
        for a in rows:
            r = out[a]
            if r is None:
                assert before['done'][a] and after['held'][a] == 0 and (not on or (after['boxed'][a] == 0 and after['box_waited'][a] == 0))
                continue
            want = (r['traj_idx'], r['cut'], r['target'], r['hit'], r['status'], r['held'])
            got = (after['traj_idx'][a], after['cut_len'][a], after['target_ind'][a], after['hit_idx'][a], after['status'][a], after['held'][a])
            assert want == tuple(int(v) for v in got), (s, a, want, got)
            worst = max(worst, float(np.abs(r['u_sol'] - after['u'][a]).max()), float(np.abs(r['x_sol'] - after['x'][a]).max()),
                        float(np.abs(r['post'] - after['state'][a]).max()))
            assert bool(after['done'][a]) == loop.done[a], (s, a)
        # the entries as the device's own words show them: occ from a rule-less look at the device's traj_idx is the oracle loop's
        entries += [(s, a) for a in KH.box_entries(before['traj_idx'], after['traj_idx'], loop.line, loop.movement, loop.kc_tab['conflict'], loop.occ_hist[-1])
                    if not before['done'][a]]
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        if after['done'].all():
            break
    assert entries == loop.entries
    return worst, boxed_steps, arr, entries


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_late_straight_on_the_oracle(ctx, stock, mode):
    """GK2.  The late-straight scene of tests/test_keepclear_cpu.py K4 in the device loop under the fixed plan, in both stop modes, until
    both cars have arrived, every step replayed on a KeepClearPlanLoop from the device's own state before the step (the loop's integers
    are never re-synchronised).  traj_idx, cut_len, held, boxed, waited, box_occupied, n_boxed, target index, hit and status are identical;
    states and solutions agree within 2e-7.  With the stage on nobody enters an occupied box, the arm-2 car is boxed and the arm-1 car never
    is; THE SAME RUN WITH THE STAGE OFF HAS SUCH AN ENTRY -- the assertion that fails without the feature."""
    speed = mode == 'speed'
    res = {}
    for on in (True, False):
        sim = _late(ctx, stock, mode, keep_clear=on)
        loop = KH.late_loop(on, speed=speed)
        worst, boxed_steps, arr, entries = _replay(sim, loop, 200)
        print('late straight, %s, keep clear %s: worst |GPU - oracle| %.2e, arrivals %s, boxed steps %s, entries %s'
              % (mode, on, worst, arr.tolist(), boxed_steps.tolist(), entries))
        assert worst < TOL, worst
        assert (arr > 0).all() and arr.tolist() == loop.arrival
        res[on] = (boxed_steps, entries, loop)
    assert res[True][1] == [] and len(res[False][1]) >= 1 and all(a == 1 for _, a in res[False][1])
    assert res[True][0][1] >= 1 and res[True][0][0] == 0 and not res[False][0].any()
    assert not any(c[4] == 'exempt' for c in res[True][2].candidates)
    assert res[True][2].worst_clearance > 0.0 and res[True][2].worst_clearance >= res[False][2].worst_clearance


def test_late_straight_under_a_controller(ctx, stock):
    """GK3.  The same under actuate(): the controller ends the first phase two steps after the arm-1 car has passed its line and gives arm
    2 green while it is crossing.  Replayed on a KeepClearActuatedLoop: the junction state and the calls are identical too -- held stays
    the signal stage's word, so the controller counts what it counted without the stage."""
    res = {}
    for on in (True, False):
        sim = _late(ctx, stock, 'cut', keep_clear=on, actuated=True)
        loop = KH.late_loop(on, controller=_controller())
        worst, boxed_steps, arr, entries = _replay(sim, loop, 200)
        print('late straight under a controller, keep clear %s: worst %.2e, arrivals %s, boxed steps %s, entries %s' % (on, worst, arr.tolist(), boxed_steps.tolist(), entries))
        assert worst < TOL and (arr > 0).all() and arr.tolist() == loop.arrival
        res[on] = (boxed_steps, entries, loop)
    assert res[True][1] == [] and len(res[False][1]) >= 1
    assert res[True][0][1] >= 1 and res[True][0][0] == 0
    # the calls up to the first entry without the rule are the same in both runs: the stage does not touch what the controller reads
    n = res[False][1][0][0]
    assert res[True][2].calls_hist[:n] == res[False][2].calls_hist[:n] and res[True][2].jstate_hist[:n] == res[False][2].jstate_hist[:n]


def _flow(c, stock, keep_clear=True):
    """the lifecycle scene of keepclear_helpers: one instance of eight slots, admission, respawn with routes, give_way('entry'), following,
    a controller, keep clear"""
    routes, dl, cd = stock
    sc, ct, tab = KH.flow_scene(routes)
    sim = GR._batch(c, stock, sc['route_of'][:, :, 0], sc['start_idx'][:, :, 0], 'cut')      # (retire_at_goal(leave_scene=True))
    sim.respawn_on_schedule(sc['due'], gap=sc['gap'], route=sc['route_of'], start_index=sc['start_idx'])
    sim.give_way('entry')
    sim.actuate(ct)
    if keep_clear:
        sim.keep_clear()
    sim.follow(**sc['follow'])
    return sim, tab


def _flow_snap(sim):
    """snapshot() and the device words it leaves out, under the names of stack_helpers and keepclear_helpers.FLOW_WORDS"""
    out = sim.snapshot()
    get = lambda t: t.cpu().numpy().copy()
    out.update(path_off=get(sim.path_off), path_len=get(sim.path_len), clock=get(sim.clock), ep_i32=get(sim.ep_i32), ep_f64=get(sim.ep_f64),
               jstate=get(sim.junction_state), calls=get(sim.calls))
    return out


def test_lifecycle_under_a_controller(ctx, stock, libs):
    """GK4.  Keep clear beside following, give_way('entry'), retirement with leave_scene=True and respawn with routes under actuate(): one
    instance of eight slots (stack_helpers' scene under a controller with min_green 8, max_green 25, gap 3, amber 3, no all-red), 150
    steps, every one before = snapshot, run(1), after = snapshot with `after` = keepclear_helpers.flow_step(before).  Integer words
    identical -- held, jstate, lights, calls, boxed, waited, box_occupied, n_boxed among them --, gap and follow_cap bit for bit, u, x,
    state and applied within 2e-7.  The run has three phase changes, boxed cars of every slot, candidates that waited and candidates that
    could stop, slots reset and served again with their waited word healed, and no entry into an occupied box."""
    from tests import stack_helpers as K
    sim, tab = _flow(ctx, stock)
    cfg, first = KH.flow_config(libs, K.stock_paths()[0], K.stock_paths()[1])
    assert np.array_equal(sim.path.cpu().numpy(), cfg.path) and sim.dl == cfg.dl
    for k, name in (('path_move', 'path_move'), ('path_exit', 'path_exit'), ('conflict', 'conflict')):
        assert np.array_equal(sim._keepclear_tabs[k].cpu().numpy(), cfg.keepclear[name]), k
    assert sim._keepclear.detect == cfg.keepclear['detect'] and sim._signals.brake == cfg.hold['brake']
    assert np.array_equal(sim._signal_tabs['path_stop'].cpu().numpy(), cfg.hold['path_stop'])
    before = _flow_snap(sim)
    for k in K.INT_WORDS + KH.FLOW_WORDS:
        if k in first and k in before:
            assert np.array_equal(first[k], before[k]), k
    worst, boxed, why, entries, phases, healed = 0.0, np.zeros(cfg.P, np.int64), {}, [], [], 0
    for s in range(KH.FLOW_STEPS):
        sim.run(1)
        after = _flow_snap(sim)
        want, info = KH.flow_step(cfg, before)
        worst = max(worst, K.compare_words(after, want, cfg, what=s))
        for k in KH.FLOW_WORDS:
            assert np.array_equal(after[k], want[k]), (s, k, after[k], want[k])
        boxed += after['boxed'] != 0
        for c in info['candidates']:
            why[c[4]] = why.get(c[4], 0) + 1
        entries += [(s, q) for q in info['entries']]
        phases.append(int(after['jstate'][0][0]))
        healed += sum(1 for q in info['admitted'] if before['served'][q] > 0 and not before['box_waited'][q])
        before = after
    sim.check()
    changes = sum(1 for a, b in zip(phases, phases[1:]) if a != b)
    print('lifecycle under a controller: worst |GPU - oracle| %.2e, boxed steps %s, candidates %s, phase changes %d, served %s'
          % (worst, boxed.tolist(), why, changes, before['served'].tolist()))
    assert entries == [] and changes >= 2 and (boxed > 0).all() and why.get('waited', 0) > 0 and why.get('can stop', 0) > 0
    assert before['served'].sum() >= cfg.P and healed >= 1


# ---------------------------------------------------------------- GK5
def test_graph_replay_and_host_staging(ctx, stock):
    """GK5.  8 chunks of run(5, graph=True) on a side stream equal 40 x run(1) plain, byte for byte, boxed, waited, box_occupied and n_boxed
    included; step_staged() -- the per-stage entry points with mpcx_keepclear_step_batch behind the signal / actuated stage call --
    equals run(1) after every one of 40 steps on the loop without retirement, under the plan and under the controller.  The 40 steps
    span the arm-2 car's wait at red, its steps boxed and its release."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _late(ctx, stock)
    seen = set()
    for _ in range(40):
        plain.run(1)
        seen.add((int(plain.box_occupied[0]), int(plain.n_boxed[0])))
    a = _snap(plain)
    assert {(0, 0), (2, 0), (2, 1)} <= seen
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _late(side, stock)
        torch.cuda.synchronize()
        for _ in range(8):
            graph.run(5, graph=True)
        _same(_snap(graph), a, 'graph')
    finally:
        side.close()
    for actuated in (False, True):
        X, Y = (_late(ctx, stock, actuated=actuated, retire=False) for _ in range(2))
        boxed = 0
        for s in range(40):
            X.run(1); Y.step_staged()
            x = _snap(X)
            _same(_snap(Y), x, (actuated, s))
            boxed += int(x['boxed'][1])
        assert boxed >= 10 and not x['boxed'][0]


# ---------------------------------------------------------------- GK6
def test_off_means_off(ctx, stock):
    """GK6.  keep_clear() then enter_on_green() gives the bytes of a batch that never had the stage: every buffer of snapshot(), sol and
    the run log, under the plan and under the controller (45 steps: past the entry the stage would have prevented).  With an all-zero
    conflict table the stage is on and writes its own words, and everything else equals the plain run.  unsignalise() and reserve()
    switch the stage off with the signals."""
    for actuated in (False, True):
        base = _late(ctx, stock, keep_clear=False, actuated=actuated)
        base.attach_log(45)
        base.run(45)
        want, rows = _snap(base), base.log.rows()
        sim = _late(ctx, stock, actuated=actuated)
        sim.enter_on_green()
        assert sim._keepclear is None and sim._signals is not None
        sim.attach_log(45)
        sim.run(45)
        got = _snap(sim)
        assert 'boxed' not in got and 'box_occupied' not in got
        _same(got, want, 'enter_on_green')
        assert sim.log.rows().tobytes() == rows.tobytes()
        assert not sim.boxed.any() and not sim.box_waited.any() and not sim.box_occupied.any()      # no longer written
        zero = _late(ctx, stock, keep_clear=False, actuated=actuated)
        zero.keep_clear(conflict=np.zeros(12, dtype=np.int32))
        zero.attach_log(45)
        seen = set()
        for _ in range(45):
            zero.run(1)
            seen.add(int(zero.box_occupied[0]))
        got = _snap(zero)
        own = ('boxed', 'box_waited', 'box_occupied', 'n_boxed')
        assert all(k in got for k in own) and not got['boxed'].any() and {0, 2, 18} <= seen
        _same({k: v for k, v in got.items() if k not in own}, want, 'zero table')
        assert zero.log.rows().tobytes() == rows.tobytes()
        on = _late(ctx, stock, actuated=actuated); on.run(45)
        assert _snap(on)['state'].tobytes() != want['state'].tobytes()
    sim = _late(ctx, stock)
    sim.unsignalise()
    assert sim._keepclear is None and sim._signals is None and 'boxed' not in sim.snapshot()
    sim = _late(ctx, stock)
    sim.reserve(dict(detect=144, patience=0))
    assert sim._keepclear is None and sim._reservation is not None
    sim.run(3)
    sim = _late(ctx, stock)        # signalise() <-> actuate(): the signals are replaced, not removed, and the stage stays
    sim.actuate(_controller())
    assert sim._keepclear is not None
    sim.run(3)


# ---------------------------------------------------------------- GK7
def _run_entry(sim, n, graph=0, signals='own', reservation=None, **over):
    """the widest entry point itself with the structs of `sim` unless given (the stage is the context's: _claim_context sets it)"""
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, retire=sim._retire, scene=sim._scene)
    st.update(over)
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    sg = sim._signals if isinstance(signals, str) else signals
    c._chk(c.lib.mpcx_closed_loop_run_reserved(c._ctx, C.byref(cip), C.byref(st['desc']), None, byref(sim._opts), byref(st['retire']),
                                               byref(st['scene']), byref(sim._admit), byref(sim._respawn), byref(sim._routes),
                                               byref(sim._precedence), byref(sg), byref(sim._actuation), None, None, byref(reservation),
                                               int(n), int(graph)))


def test_refusals(ctx, stock):
    """GK7.  MPCX_E_INVALID with a "keepclear: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: no signals in the run, a reservation in the run, a NULL pointer among the seven, n_per outside 1..64, n_per
    n_junctions != P, n_moves outside 1..16, n_points not the signals', detect < 1, a conflict word with bits at or above n_moves, with its
    own bit or asymmetric, more than one linearisation pass, the agent-sharded layout, a nonzero reserved word; the stage-level call
    refuses the same way.  In Python: keep_clear() without signals, under reserve(), with malformed tables."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _late(ctx, stock)
    before = _snap(sim)
    sg, kc = sim._signals, sim._keepclear
    names = [n for n, _ in _lib.KeepClearC._fields_]
    good = {n: getattr(kc, n) for n in names}
    make = lambda **kw: _lib.KeepClearC(**dict(good, **kw))
    keep = []

    def refused(match, struct, **over):
        for graph in (0, 1):
            for n in (0, 1):
                sim._claim_context()
                ctx.set_keepclear(struct)
                try:
                    with pytest.raises(MpcxError, match=match):
                        _run_entry(sim, n, graph, **over)
                finally:
                    ctx.set_keepclear(None)
    for n in names[:7]:
        refused(r'mpcx error -1: keepclear: %s is null' % n, make(**{n: None}))
    refused(r'mpcx error -1: keepclear: the reserved word is not 0', make(reserved=1))
    refused(r'mpcx error -1: keepclear: needs signals', kc, signals=None)
    rsv = _late(ctx, stock, keep_clear=False); rsv.reserve(dict(detect=144, patience=0))
    refused(r'mpcx error -1: keepclear: the run also carries a reservation', kc, signals=rsv._signals, reservation=rsv._reservation)
    for n in (0, -2, 65):
        refused(r'mpcx error -1: keepclear: n_per = %d outside 1\.\.64' % n, make(n_per=n))
    refused(r'mpcx error -1: keepclear: n_per \* n_junctions = 2 \* 3 is not P = 2', make(n_junctions=3))
    refused(r'mpcx error -1: keepclear: n_per \* n_junctions = 1 \* 1 is not P = 2', make(n_per=1))
    for n in (0, 17):
        refused(r'mpcx error -1: keepclear: n_moves = %d outside 1\.\.16' % n, make(n_moves=n))
    refused(r'mpcx error -1: keepclear: n_points = %d is not the signals\' %d' % (kc.n_points - 1, kc.n_points), make(n_points=kc.n_points - 1))
    for d in (0, -3):
        refused(r'mpcx error -1: keepclear: detect = %d' % d, make(detect=d))
    stock_cf = sim._keepclear_tabs['conflict'].cpu().numpy().astype(np.int64)
    assert len(stock_cf) == 12 and stock_cf[1] & (1 << 4) and not stock_cf[1] & (1 << 7)       # straight from arm 1 against from arm 2 / arm 3

    def table(cf, **kw):
        t = ctx.i32(np.asarray(cf))
        ctx.synchronize()
        keep.append(t)
        return make(conflict=t.data_ptr(), **kw)
    edit = lambda g, v: np.concatenate([stock_cf[:g], [v], stock_cf[g + 1:]])
    refused(r'mpcx error -1: keepclear: conflict is not symmetric at movements 1 and 4', table(edit(1, stock_cf[1] & ~(1 << 4))))
    refused(r'mpcx error -1: keepclear: movement 3 conflicts with itself', table(edit(3, stock_cf[3] | 8)))
    refused(r'mpcx error -1: keepclear: movement 0 has conflict = 0x%x with bits at or above n_moves = 12' % (stock_cf[0] | 1 << 12), table(edit(0, stock_cf[0] | 1 << 12)))
    refused(r'mpcx error -1: keepclear: movement \d+ has conflict = 0x[0-9a-f]+ with bits at or above n_moves = 4', table(stock_cf, n_moves=4))
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 1, 2, sim.obs6.data_ptr()
    refused(r'mpcx error -1: keepclear: not supported in the agent-sharded layout', kc, desc=shard, retire=None, scene=None)
    ctx.set_linearisation_passes(2)
    try:
        sim.lin_passes = 2
        refused(r'mpcx error -1: keepclear: 2 linearisation passes', kc, retire=None, scene=None)
        with pytest.raises(MpcxError, match='keepclear: 2 linearisation passes'):
            ctx.keepclear_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg, kc)
    finally:
        sim.lin_passes = 1
        ctx.set_linearisation_passes(1)
    # the stage-level call refuses the same way, before its launch
    for bad, match in ((make(boxed=None), 'boxed is null'), (make(n_per=70), 'n_per = 70'), (make(n_junctions=5), r'is not P = 2'), (make(detect=0), 'detect = 0'),
                       (make(reserved=3), 'reserved word'), (table(edit(3, stock_cf[3] | 8)), 'conflicts with itself')):
        with pytest.raises(MpcxError, match='keepclear: .*' + match):
            ctx.keepclear_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg, bad, done=sim.done)
    with pytest.raises(MpcxError, match='keepclear: needs signals'):
        ctx.keepclear_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], None, kc)
    ctx.synchronize()
    _same(_snap(sim), before, 'refused')
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # the limits themselves are accepted
    ctx.set_keepclear(make(detect=1)); _run_entry(sim, 0); ctx.set_keepclear(None)
    # ---- Python
    n = int(sim.path.shape[0])
    for kw in (dict(move=np.zeros(n, dtype=np.int32)), dict(move=np.zeros(3, dtype=np.int32), exit=np.zeros(3, dtype=np.int32)),
               dict(conflict=np.zeros(17, dtype=np.int32)), dict(conflict=np.zeros((2, 6), dtype=np.int32)), dict(conflict=np.zeros(12)), dict(detect=0)):
        with pytest.raises(ValueError):
            sim.keep_clear(**kw)
    assert sim._keepclear is kc
    bare = GR._batch(ctx, stock, LATE_ROUTES, np.array([KH.LATE_START[False]]), 'cut')
    with pytest.raises(ValueError, match='needs signalise'):
        bare.keep_clear()
    with pytest.raises(ValueError, match='reserve'):
        rsv.keep_clear()
    sim.unsignalise()
    assert sim._keepclear is None and 'boxed' not in sim.snapshot()


# ---------------------------------------------------------------- GK8
def test_changed_struct_under_graph_replay(stock):
    """GK8.  The cached graph's key covers the struct by value.  Another detect: the speed-mode scene, 2 steps replayed with the whole
    approach as the detector, then detect changed in place to 5 points (the arm-2 car, 13 points before its line when its light turns
    green, is no candidate until it is within 5) and 35 more replayed.  Another conflict table pointer: the cut-mode scene, 10 steps, then
    an all-zero table at another address, 35 more.  Both equal the same sequence run plain, byte for byte -- and differ from the run
    under the first struct."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        for change in ('detect', 'conflict'):
            sims = [_late(side, stock, 'speed' if change == 'detect' else 'cut') for _ in range(3)]
            torch.cuda.synchronize()
            tabs = []
            for sim, graph, changed in zip(sims, (True, False, True), (True, True, False)):
                sim.run(2 if change == 'detect' else 10, graph=graph)
                if changed and change == 'detect':
                    sim._keepclear.detect = 5
                elif changed:
                    tabs.append(side.i32(np.zeros(12, dtype=np.int32)))
                    side.synchronize()
                    sim._keepclear.conflict = tabs[-1].data_ptr()
                for _ in range(7):
                    sim.run(5, graph=graph)
            a, b, c = (_snap(sim) for sim in sims)
            _same(a, b, 'changed ' + change)
            assert a['state'].tobytes() != c['state'].tobytes(), change
    finally:
        side.close()
