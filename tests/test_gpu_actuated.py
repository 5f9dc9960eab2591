"""GPU tests of VEHICLE-ACTUATED SIGNALS in the device-resident closed loop (mpcx_closed_loop_run_actuated, IntersectionBatch.actuate):
actuated_signal_kernel takes the place of signal_kernel -- a lane group per junction reduces who is waiting in front of which line, runs
the junction's controller and holds the junction's agents with the signal rule's own hold.  The stage call against the host build of the
rule on the hand-made junctions of tests/test_actuated_cpu.py at every lane-group size; the closed loop against ActuatedOracleLoop with two
controllers in one batch; graph replay, host staging, the routed respawn batch against the host build, off means off, the refusals.
B = 2, A = 4, T = 13, v0 = 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actuated_helpers as AH
from tests import signal_helpers as G
from tests import test_gpu_respawn as GR
from tests import test_gpu_route as TR

pytestmark = pytest.mark.gpu

STRAIGHT = np.tile(np.array([1, 3, 5, 7]), (2, 1))         # the four straight stock routes
# the two controllers of the closed-loop runs: instance 0 runs tests/test_actuated_cpu.py's, instance 1 a quicker one
QUICK = dict(min_green=6, max_green=25, gap=3, amber=5, all_red=9)


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
    return AH.build_ref(tmp_path_factory.mktemp('actuated_ref'))


def _controllers():
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller
    d = AH.line_index()
    return [two_phase_controller(detect=d, **AH.CONTROLLER), two_phase_controller(detect=d, **QUICK)]


def _straight(c, stock, actuated=True, retire=True):
    """B = 2 instances of the four straight routes from index 0, cut mode; instance b under controller b"""
    sim = GR._batch(c, stock, STRAIGHT, np.zeros((2, 4), dtype=np.int64), 'cut')
    if not retire:
        sim.keep_driving()
    if actuated:
        sim.actuate(_controllers(), ctrl_of=np.array([0, 1]))
    return sim


def _snap(sim):
    out = sim.snapshot()
    if sim._actuation is not None:
        out['jstate'], out['calls'] = sim.junction_state.cpu().numpy().copy(), sim.calls.cpu().numpy().copy()
    return out


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in b:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---------------------------------------------------------------- GA1
def _device_stage(c, w):
    """mpcx_actuated_step_batch on the words of actuated_helpers.words(); returns OUT_KEYS as the device left them"""
    from mpc_for_av_at_intersection_amd import _lib
    d = {k: c.i32(w[k]) for k in AH.I32_KEYS}
    state = c.f64(w['state'])
    done = None if w['done'] is None else c.i32(w['done'])
    n_ctrl, n_phases = w['phase_groups'].shape
    sg = _lib.SignalsC(d['path_stop'].data_ptr(), d['path_group'].data_ptr(), None, None, None, None, None, d['held'].data_ptr(), float(w['brake']),
                       len(w['path_stop']), 0, int(w['n_groups']), 0)
    ac = _lib.ActuationC(d['phase_groups'].data_ptr(), d['phase_time'].data_ptr(), d['ctrl_time'].data_ptr(), d['ctrl_of'].data_ptr(),
                         d['jstate'].data_ptr(), d['lights'].data_ptr(), d['calls'].data_ptr(), int(w['n_per']), len(w['ctrl_of']), n_phases, n_ctrl, 0)
    c.synchronize()
    c.actuated_step(float(w['dl']), state, d['path_off'], d['path_len'], d['traj_idx'], d['cut_len'], sg, ac, done=done)
    c.synchronize()
    got = {k: d[k].cpu().numpy() for k in AH.I32_KEYS}
    for k in AH.I32_KEYS:       # nothing but the outputs is written
        if k not in AH.OUT_KEYS:
            assert got[k].tobytes() == w[k].tobytes(), k
    assert state.cpu().numpy().tobytes() == w['state'].tobytes()
    return {k: got[k] for k in AH.OUT_KEYS}


@pytest.mark.parametrize('n_per,J', [(1, None), (3, None), (8, None), (70, None), (8, 1), (8, 33)], ids=lambda v: 'all' if v is None else str(v))
def test_stage_call_equals_the_host_build(ctx, ref, n_per, J):
    """GA1.  mpcx_actuated_step_batch on the hand-made junctions equals the host build byte for byte -- jstate, lights, calls, held,
    cut_len -- and the values written down by hand, with and without the retirement words: n_per = 1 (a lane per junction), 3 (a padding
    lane in every group of 4), 8, 70 (a wavefront per junction, its stride loop reaches the last slot in the second round); one junction
    alone (the max-out contest); 33 junctions of 8 = five wavefronts, the last with one live group of eight."""
    w, want = AH.hand_made(n_per)
    if J == 1:
        j0 = next(i for i, c in enumerate(AH.CASES) if c[0].startswith('max-out'))
        w = AH.junctions(w, j0, j0 + 1)
    elif J is not None:
        w = AH.junctions(w, 0, J)
    assert J is None or len(w['ctrl_of']) == J
    for with_done in (True, False):
        host = AH.copy_words(w)
        if not with_done:
            host['done'] = None
        got = _device_stage(ctx, host)
        n = AH.host_rule(ref, host)
        for k in AH.OUT_KEYS:
            assert got[k].tobytes() == host[k].tobytes(), (k, with_done, np.flatnonzero((got[k] != host[k]).reshape(len(got[k]), -1).any(axis=1)))
        assert n == int((got['held'] != 0).sum())
        if with_done and J is None:
            AH.check_against_want(dict(got), want, w)


# ---------------------------------------------------------------- GA2
def _sync(loop, before, rows):
    """the oracle loop's continuous words from the device's before the step (the integers -- held, the junction state -- run on their own)"""
    loop.state, loop.applied = before['state'][rows].copy(), before['applied'][rows].copy()
    loop.traj_idx, loop.target = [int(v) for v in before['traj_idx'][rows]], [int(v) for v in before['target_ind'][rows]]
    loop.prev = [int(v) for v in before['prev_cut'][rows]]
    loop.u = [before['u'][p].copy() for p in rows]


def test_closed_loop_on_the_oracle(ctx, stock):
    """GA2.  The straight scene, cut mode, departure on, two different controllers in one batch, until everybody has arrived.  Every step
    is replayed on one ActuatedOracleLoop per instance from the device's own state before the step (the pattern of tests/test_gpu_signal.py;
    the loop's integers -- held, jstate -- are never re-synchronised).  For every driving agent held, cut_len, traj_idx, target index and
    status are identical, as are jstate, lights and calls of both junctions; states and solutions agree within 2e-7.  Not vacuous: agents
    are held and released, both junctions change phase, and the two controllers give different runs."""
    sim = _straight(ctx, stock)
    paths, dl, start, stop, group = G.straight_scene()
    loops = [AH.ActuatedOracleLoop(paths, dl, start, stop, group, ct, T=13, depart=True) for ct in _controllers()]
    worst, held_steps, phases = 0.0, np.zeros(8, dtype=np.int64), [set(), set()]
    arr = np.full(8, -1)
    for s in range(260):
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
            assert tuple(after['jstate'][b]) == tuple(loop.jstate) and after['lights'][b] == loop.lights_hist[-1] and \
                after['calls'][b] == loop.calls_hist[-1], (s, b, after['jstate'][b], loop.jstate)
            assert after['phase'][b] == loop.jstate[0] and after['stage'][b] == loop.jstate[1]
            phases[b].add(loop.jstate[:2])
            for a, p in enumerate(rows):
                r = out[a]
                if r is None:
                    assert before['done'][p] and after['held'][p] == 0
                    continue
                want = (r['traj_idx'], r['cut'], r['target'], r['hit'], r['status'], r['held'])
                got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p])
                assert want == tuple(int(v) for v in got), (s, p, want, got)
                worst = max(worst, float(np.abs(r['u_sol'] - after['u'][p]).max()), float(np.abs(r['x_sol'] - after['x'][p]).max()),
                            float(np.abs(r['post'] - after['state'][p]).max()))
                held_steps[p] += r['held'] != 0
                assert bool(after['done'][p]) == loop.done[a], (s, p)
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        if after['done'].all():
            break
    print('actuated closed loop: worst |GPU - oracle| %.2e over %d steps, arrivals %s, held steps %s' % (worst, s + 1, arr.tolist(), held_steps.tolist()))
    assert worst < 2e-7, worst
    assert after['done'].all() and after['absent'].all() and not after['held'].any()
    assert arr[:4].tolist() == loops[0].arrival and arr[4:].tolist() == loops[1].arrival and arr[:4].tolist() != arr[4:].tolist()
    assert (held_steps[[1, 3, 5, 7]] > 10).all() and not held_steps[[0, 2, 4, 6]].any()
    assert all({(0, 0), (0, 1), (0, 2), (1, 0)} <= ph for ph in phases)


# ---------------------------------------------------------------- GA3
def test_graph_replay_in_chunks(ctx, stock):
    """GA3.  15 chunks of run(7, graph=True) on a side stream equal 105 x run(1) plain, byte for byte, jstate, lights, calls and held
    included: the junction state lives in device memory, so the one captured step keeps counting"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _straight(ctx, stock)
    seen = set()
    for _ in range(105):
        plain.run(1)
        seen.add(tuple(plain.junction_state.cpu().numpy()[:, :2].reshape(-1).tolist()))
    a = _snap(plain)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _straight(side, stock)
        torch.cuda.synchronize()
        for _ in range(15):
            graph.run(7, graph=True)
        _same(a, _snap(graph), 'graph')
        assert len(seen) >= 4 and a['done'].any()
    finally:
        side.close()


# ---------------------------------------------------------------- GA4
def test_host_staging_equals_the_loop(ctx, stock):
    """GA4.  step_staged() -- the per-stage entry points with mpcx_actuated_step_batch between the conflict search and the window stage --
    equals run(1) after every one of 40 steps, the junction words and held included, on the plain loop without retirement"""
    X, Y = (_straight(ctx, stock, retire=False) for _ in range(2))
    held = np.zeros(8, dtype=np.int64)
    for s in range(40):
        X.run(1); Y.step_staged()
        x = _snap(X)
        _same(x, _snap(Y), s)
        held += x['held'] != 0
    assert (held[[1, 3, 5, 7]] > 10).all() and not held[[0, 2, 4, 6]].any() and x['jstate'][:, :2].tolist() == [[0, 2], [1, 0]]      # (as the CPU oracle's runs: all red / the second green)


# ---------------------------------------------------------------- GA5
def test_routed_respawn_batch_follows_the_host_rule(ctx, stock, ref):
    """GA5.  The routed respawn batch of tests/test_gpu_route.py (B = 2) under a short two-phase controller, 100 steps.  After every step
    jstate, lights, calls, held and cut_len equal the host build of the rule applied to the device's own words of that step: traj_idx as
    the step left it, the state, held and jstate before the step, the tables, and for the cut the conflict search's own (the path length
    where it found no conflict; where it found one the rule can only have lowered it, which is checked as such).  An agent that arrives in
    the step is past its line and calls nothing; respawn may have reset its slot's words already, so it goes into the host rule as done."""
    from mpc_for_av_at_intersection_amd.batch import stop_lines, two_phase_controller
    sim = TR._routed(ctx, stock)
    stop, group = stop_lines(stock[0], setback=1.0)         # (the batch starts 3 m before the crossing: a line between start and crossing)
    sim.actuate([two_phase_controller(4, 12, 3, 4, 2, detect=12), two_phase_controller(3, 9, 2, 2, 3, detect=6)], ctrl_of=np.array([0, 1]),
                stop=stop, group=group)
    tabs = {k: v.cpu().numpy() for k, v in sim._signal_tabs.items()}
    seen, stages, lowered = set(), set(), 0
    for s in range(100):
        before = _snap(sim)
        b_off, b_len = sim.path_off.cpu().numpy().copy(), sim.path_len.cpu().numpy().copy()
        sim.run(1)
        after = _snap(sim)
        admitted = (before['entered_step'] < 0) & (after['entered_step'] >= 0)
        assert not before['held'][admitted].any(), s
        driving = (before['done'] == 0) | admitted
        arrived = driving & (after['done'] != 0)              # (respawn may have reset this slot's words already)
        keep = driving & ~arrived
        cut_in = np.where(after['hit_idx'] >= 0, after['cut_len'], b_len).astype(np.int32)
        w = AH.words(state=before['state'], path_off=b_off, path_len=b_len, traj_idx=after['traj_idx'], cut_len=cut_in,
                     done=(~keep).astype(np.int32), held=before['held'], jstate=before['jstate'], lights=np.zeros(2), calls=np.zeros(2),
                     dl=sim.dl, brake=float(sim._signals.brake), n_groups=int(sim._signals.n_groups), n_per=sim.A, **tabs)
        AH.host_rule(ref, w)
        for k in ('jstate', 'lights', 'calls'):
            assert np.array_equal(w[k], after[k]), (s, k, w[k], after[k])
        assert np.array_equal(w['held'][~arrived], after['held'][~arrived]) and not after['held'][arrived].any(), (s, w['held'], after['held'])
        assert np.array_equal(w['cut_len'][keep], after['cut_len'][keep]), (s, w['cut_len'], after['cut_len'])
        hk = keep & (after['held'] != 0)
        line = tabs['path_stop'][(b_off + after['traj_idx'])[hk]]
        assert (after['cut_len'][hk] <= line).all() and (after['traj_idx'][hk] < line).all(), s
        lowered += int((after['cut_len'][hk] == line).sum())
        seen |= set(after['held'].tolist())
        stages |= {tuple(v) for v in after['jstate'][:, :2].tolist()}
    print('routed respawn, actuated: held values seen %s, %d agent-steps cut at the line, junction (phase, stage) seen %s' %
          (sorted(seen), lowered, sorted(stages)))
    assert seen >= {0, 1} and lowered > 10 and len(stages) >= 4


# ---------------------------------------------------------------- GA6
def _entry(sim, signals, actuation, n, graph=0, **over):
    """mpcx_closed_loop_run_actuated itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, retire=sim._retire, scene=sim._scene)
    st.update(over)
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_actuated(c._ctx, C.byref(cip), C.byref(st['desc']), None, byref(sim._opts), byref(st['retire']),
                                               byref(st['scene']), byref(sim._admit), byref(sim._respawn), byref(sim._routes),
                                               byref(sim._precedence), byref(signals), byref(actuation), int(n), int(graph)))


def test_off_means_off(ctx, stock):
    """GA6.  After unsignalise() the run equals a batch that never had signals, bit for bit (40 steps); actuation = NULL and an all-zero
    struct through mpcx_closed_loop_run_actuated give the bytes of mpcx_closed_loop_run_signals with the same fixed plan; signalise() after
    actuate() and the reverse replace the source of the lights"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    base = _straight(ctx, stock, actuated=False)
    base.run(40)
    want = base.snapshot()
    sim = _straight(ctx, stock)
    sim.unsignalise()
    assert sim._actuation is None and sim._signals is None
    sim.run(40)
    got = sim.snapshot()
    assert 'held' not in got and 'phase' not in got
    _same(got, want, 'unsignalise')
    assert not sim.junction_state.any() and not sim.held.any()        # no longer read or written
    act = _straight(ctx, stock); act.run(40)
    assert act.snapshot()['state'].tobytes() != want['state'].tobytes() and act.snapshot()['held'].any()
    # a fixed plan with no actuation: the signals' own run
    plan = two_phase_plan(**G.PLAN)
    fixed = _straight(ctx, stock, actuated=False); fixed.signalise(plan); fixed.run(40)
    want = fixed.snapshot()
    for name, ac in (('NULL', None), ('zero struct', _lib.ActuationC())):
        sim = _straight(ctx, stock, actuated=False); sim.signalise(plan)
        _entry(sim, sim._signals, ac, 40)
        _same(sim.snapshot(), want, name)
    sim = _straight(ctx, stock); sim.signalise(plan)            # signalise() after actuate()
    assert sim._actuation is None
    sim.run(40)
    _same(sim.snapshot(), want, 'signalise after actuate')
    sim = _straight(ctx, stock, actuated=False); sim.signalise(plan); sim.actuate(_controllers(), ctrl_of=np.array([0, 1]))
    sim.run(40)
    _same(_snap(sim), _snap(act), 'actuate after signalise')


# ---------------------------------------------------------------- GA7
def test_refusals(ctx, stock):
    """GA7.  MPCX_E_INVALID with an "actuation: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: a NULL pointer, actuation without signals, signals that also carry a fixed plan, n_per < 1, n_per n_junctions
    != P, n_phases outside 1..8, n_ctrl < 1, a nonzero reserved word, a phase mask that is zero or has a bit at or above n_groups, min_green
    < 0, max_green < 1, min_green > max_green, gap < 1, amber < 0, all_red < 0, detect < 1, the agent-sharded layout, more than one
    linearisation pass; the stage-level call refuses the same way.  In Python: malformed controllers and tables."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _straight(ctx, stock)
    before = _snap(sim)
    sg, ac = sim._signals, sim._actuation
    names = [n for n, _ in _lib.ActuationC._fields_]
    good = {n: getattr(ac, n) for n in names}
    make = lambda **kw: _lib.ActuationC(**dict(good, **kw))

    def refused(match, actuation, signals=sg, **over):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _entry(sim, signals, actuation, n, graph, **over)
    for n in names[:7]:
        refused(r'mpcx error -1: actuation: %s is null' % n, make(**{n: None}))
    refused(r'mpcx error -1: actuation: needs signals', ac, signals=None)
    planned = _straight(ctx, stock, actuated=False); planned.signalise(two_phase_plan(**G.PLAN))
    refused(r'mpcx error -1: actuation: the signals also carry a fixed plan', ac, signals=planned._signals)
    sg_names = [n for n, _ in _lib.SignalsC._fields_]
    sgood = {n: getattr(sg, n) for n in sg_names}
    refused(r'mpcx error -1: actuation: signals\.held is null', ac, signals=_lib.SignalsC(**dict(sgood, held=None)))
    refused(r'mpcx error -1: actuation: signals\.n_groups = 17 outside 1\.\.16', ac, signals=_lib.SignalsC(**dict(sgood, n_groups=17)))
    for n in (0, -2):
        refused(r'mpcx error -1: actuation: n_per = %d' % n, make(n_per=n))
    refused(r'mpcx error -1: actuation: n_per \* n_junctions = 4 \* 3 is not P = 8', make(n_junctions=3))
    refused(r'mpcx error -1: actuation: n_per \* n_junctions = 8 \* 2 is not P = 8', make(n_per=8))
    for n in (0, 9):
        refused(r'mpcx error -1: actuation: n_phases = %d outside 1\.\.8' % n, make(n_phases=n))
    refused(r'mpcx error -1: actuation: n_ctrl = 0', make(n_ctrl=0))
    refused(r'mpcx error -1: actuation: a reserved word is not 0', make(reserved=1))

    def tables(masks=(5, 10), times=((10, 40, 5), (10, 40, 5)), ctrl=(8, 12, 100)):
        t = (ctx.i32(np.array([masks])), ctx.i32(np.array([times])), ctx.i32(np.array([ctrl])))
        ctx.synchronize()
        return t, make(phase_groups=t[0].data_ptr(), phase_time=t[1].data_ptr(), ctrl_time=t[2].data_ptr(), n_ctrl=1)
    zero_of = ctx.i32(np.zeros(2))
    for kw, match in ((dict(masks=(5, 0)), r'controller 0 phase 1 has group mask = 0x0'),
                      (dict(masks=(21, 10)), r'controller 0 phase 0 has group mask = 0x15'),
                      (dict(times=((-1, 40, 5), (10, 40, 5))), r'controller 0 phase 0 has min_green = -1'),
                      (dict(times=((0, 0, 5), (10, 40, 5))), r'controller 0 phase 0 has max_green = 0'),
                      (dict(times=((10, 40, 5), (41, 40, 5))), r'controller 0 phase 1 has min_green = 41 > max_green = 40'),
                      (dict(times=((10, 40, 0), (10, 40, 5))), r'controller 0 phase 0 has gap = 0'),
                      (dict(ctrl=(-1, 12, 100)), r'controller 0 has amber = -1'),
                      (dict(ctrl=(8, -3, 100)), r'controller 0 has all_red = -3'),
                      (dict(ctrl=(8, 12, 0)), r'controller 0 has detect = 0')):
        keep, bad = tables(**kw)
        bad.ctrl_of = zero_of.data_ptr()
        refused(r'mpcx error -1: actuation: ' + match, bad)
    keep, fine = tables(masks=(15, 8), times=((0, 1, 1), (40, 40, 1)), ctrl=(0, 0, 1))       # the limits themselves are accepted
    fine.ctrl_of = zero_of.data_ptr()
    _entry(sim, sg, fine, 0)
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 2, 4, sim.obs6.data_ptr()
    refused(r'mpcx error -1: actuation: not supported in the agent-sharded layout', ac, desc=shard, retire=None, scene=None)
    ctx.set_linearisation_passes(2)
    try:
        sim.lin_passes = 2
        refused(r'mpcx error -1: actuation: 2 linearisation passes', ac, retire=None, scene=None)
        with pytest.raises(MpcxError, match='actuation: 2 linearisation passes'):
            ctx.actuated_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg, ac)
    finally:
        sim.lin_passes = 1
        ctx.set_linearisation_passes(1)
    # the stage-level call refuses the same way, before its launch
    for bad, match in ((make(jstate=None), 'jstate is null'), (make(n_phases=40), 'n_phases = 40'), (make(n_junctions=5), r'is not P = 8'),
                       (tables(ctrl=(8, 12, -4))[1], 'detect = -4')):
        with pytest.raises(MpcxError, match='actuation: .*' + match):
            ctx.actuated_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg, bad, done=sim.done)
    with pytest.raises(MpcxError, match='actuation: the signals also carry a fixed plan'):
        ctx.actuated_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], planned._signals, ac)
    ctx.synchronize()
    _same(_snap(sim), before, 'refused')
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # ---- Python
    ct = _controllers()[0]
    n = int(sim.path.shape[0])
    for kw in (dict(controllers=[]), dict(controllers=[ct, dict(ct, phases=[[0, 1, 2, 3]])]), dict(controllers=dict(ct, phases=[[0], []])),
               dict(controllers=dict(ct, phases=[[0], [16]])), dict(controllers=dict(ct, phases=[[g] for g in range(9)])),
               dict(controllers=dict(ct, gap=[1, 2, 3])), dict(controllers=dict(ct, min_green=2.5)),
               dict(controllers=ct, stop=np.zeros(n, dtype=np.int32)), dict(controllers=ct, stop=np.zeros(3, dtype=np.int32), group=np.zeros(3, dtype=np.int32)),
               dict(controllers=ct, ctrl_of=np.zeros(8, dtype=np.int64)), dict(controllers=ct, ctrl_of=np.zeros(2))):
        with pytest.raises(ValueError):
            sim.actuate(**kw)
    assert sim._actuation is ac and sim._signals is sg
    sim.unsignalise()
    assert sim._actuation is None and sim._signals is None and 'phase' not in sim.snapshot()
