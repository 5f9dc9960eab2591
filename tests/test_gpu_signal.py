"""GPU tests of TRAFFIC SIGNALS in the device-resident closed loop (mpcx_closed_loop_run_signals, IntersectionBatch.signalise): one launch
behind the conflict search holds an agent whose light is red -- or amber, if it can stop -- at its stop line by lowering its cut length (its
stop index in speed mode) to the line.  The defining property: every driving agent of every step equals the oracle step in which the cut
the conflict search produced is replaced by its minimum with the line for a held agent (signal_helpers.signal_agent_step) -- on the scene
tests/test_signal_cpu.py pins on the CPU oracle alone.  Then: plans as a sweep, all green is the run without signals, off means off, graph
replay, host staging, the rule on a routed respawn batch, signals with right of way, the refusals.  B = 2, A = 4, T = 13, v0 = 0."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import scene_helpers as SH
from tests import signal_helpers as G
from tests import test_gpu_respawn as GR
from tests import test_gpu_route as TR
from tests import test_gpu_scene as GS

pytestmark = pytest.mark.gpu

T = GR.T
KEYS = GS.KEYS
STRAIGHT = np.tile(np.array([1, 3, 5, 7]), (2, 1))         # the four straight stock routes
# the two plans of the sweep (cut mode, on the CPU oracle): instance 0 meets amber too close to its line to stop, instance 1 is held at amber
SWEEP = (dict(cycle=80, green=20, amber=10), dict(cycle=120, green=35, amber=8))
SWEEP_OFFSET = (3, 36)


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
    return G.build_ref(tmp_path_factory.mktemp('signal_ref'))


def _plans(*specs):
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    return [two_phase_plan(**s) for s in specs]


def _straight(c, stock, mode='cut', plans=(G.PLAN,), plan_of=None, offset=None, retire=True):
    """B = 2 instances of the four straight routes from index 0; plans: two_phase_plan arguments, None = no signals"""
    sim = GR._batch(c, stock, STRAIGHT, np.zeros((2, 4), dtype=np.int64), mode)
    if not retire:
        sim.keep_driving()
    if plans is not None:
        sim.signalise(_plans(*plans), plan_of=plan_of, offset=offset)
    return sim


def _tables(sim):
    t = {k: v.cpu().numpy() for k, v in sim._signal_tabs.items()}
    t['brake'] = float(sim._signals.brake)
    return t


def _snap(sim):
    out = sim.snapshot()
    if sim._signals is not None:
        out['tick'] = sim.tick.cpu().numpy().copy()
    return out


def _replay_step(sim, before, after, pool, absent, tabs):
    """Every DRIVING agent of the step replayed on the oracle with the rule (signal_helpers.signal_agent_step; the obstacle list is its pool
    window minus its own row minus the absent rows).  traj_idx, cut_len, hit_idx, target_ind, status, held, done and absent identical, u and
    x within 2e-7 (the project's bar); every agent's clock has advanced; a retired agent's buffers are unchanged and it is not held.
    Returns (worst difference, agents held, agents for which the line replaced the conflict search's cut)."""
    from oracle import oracle_py as orc
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    speed = sim.stop_mode == 'speed'
    stop = sim.stop_index() if speed else None
    retire = 'done' in before
    worst, n_held, n_cut = 0.0, 0, 0
    for p in range(sim.P):
        plan = int(tabs['plan_of'][p])
        cycle = int(tabs['plan_cycle'][plan])
        t = int(before['tick'][p]) % cycle
        assert after['tick'][p] == (t + 1) % cycle, p
        if retire and before['done'][p]:
            for k in KEYS:
                if k != 'applied':
                    assert before[k][p].tobytes() == after[k][p].tobytes(), (p, k)
            assert not after['applied'][p].any() and after['held'][p] == 0
            continue
        present = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p] and not (retire and absent[r])]

        def decide(ti, v, p=p, plan=plan, cycle=cycle, t=t):
            i = int(off[p]) + ti
            s, g = int(tabs['path_stop'][i]), int(tabs['path_group'][i])
            if s < 0 or ti >= s or s >= ln[p]:
                return 0, s
            lt = G.light(cycle, int(tabs['plan_amber'][plan]), int(tabs['plan_green'][plan, g, 0]), int(tabs['plan_green'][plan, g, 1]), t)
            if lt == G.RED:
                return 1, s
            if lt == G.AMBER and (before['held'][p] != 0 or np.float64(s - ti) * np.float64(sim.dl) >= np.float64(v) * np.float64(v) / (2.0 * tabs['brake'])):
                return 2, s
            return 0, s
        r = G.signal_agent_step(po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], pool[present], int(before['traj_idx'][p]),
                                int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                                sim.ip.cutoff_margin, speed, decide, v_ref=sim.v_ref if speed else None)
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        want = (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status, r['held'])
        if speed:
            got = (after['traj_idx'][p], stop[p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p])
            assert after['cut_len'][p] == (r['cut'] if (r['hit'] is not None or r['held']) else ln[p]), p
        else:
            got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p])
        assert want == tuple(int(v) for v in got), (p, want, got)
        assert r['sol'].status == 0
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        n_held += r['held'] != 0
        n_cut += r['held'] != 0 and r['cut'] == r['line']
        if retire:      # retirement and departure as the step's last launch leaves them: mpc.is_goal on the state after the plant step
            arrived = SH.is_goal(after['state'][p], tab[off[p] + ln[p] - 1], after['target_ind'][p], ln[p] if speed else after['cut_len'][p])
            assert bool(after['done'][p]) == arrived and after['absent'][o_skip[p]] == int(arrived), (p, arrived)
    assert worst < 2e-7, worst
    return worst, n_held, n_cut


def _stepped(sim, steps):
    """run(1) + snapshot with the oracle replay of every step, until everybody has arrived; returns (arrival steps, worst, held, cut, recs)"""
    tabs = _tables(sim)
    worst, held, cut, recs = 0.0, 0, 0, []
    arr = np.full(sim.P, -1)
    for s in range(steps):
        before = _snap(sim)
        sim.run(1)
        after = _snap(sim)
        w, h, c = _replay_step(sim, before, after, GS._pool_before(sim, before, after), before['absent'], tabs)
        worst, held, cut = max(worst, w), held + h, cut + c
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        recs.append(after)
        if after['done'].all():
            break
    return arr.tolist(), worst, held, cut, recs


def _cpu_arrivals(spec, offset, speed=False):
    loop = G.straight_loop(_plans(spec)[0], tick=[offset] * 4, speed=speed)
    loop.run(600)
    return loop


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_straight_scene_on_the_oracle(ctx, stock, mode):
    """G1.  tests/test_signal_cpu.py's scene (four straight routes from index 0 under signal_helpers.PLAN, departure on) in both stop modes;
    instance 1 starts half a cycle later in the plan, so its phases are swapped.  After every step every driving agent equals the
    SignalOracleLoop step; both instances arrive at the steps of the CPU oracle's own run (cut mode: 56 / 98 / 56 / 98).  Not vacuous: agents
    are held, and the line -- not a conflict -- is what cuts their path."""
    sim = _straight(ctx, stock, mode, offset=np.array([0, 50]))
    cpu = [_cpu_arrivals(G.PLAN, o, mode == 'speed') for o in (0, 50)]
    arr, worst, held, cut, recs = _stepped(sim, 260)
    print('%s: worst |GPU - oracle| %.2e over %d steps, arrivals %s, %d agent-steps held, %d cut at the line' % (mode, worst, len(recs), arr, held, cut))
    assert arr[:4] == cpu[0].arrival and arr[4:] == cpu[1].arrival and min(arr) > 0
    if mode == 'cut':
        assert arr[:4] == [56, 98, 56, 98]
    assert held > 30 and cut > 30 and recs[-1]['absent'].all() and not recs[-1]['held'].any()


# ---------------------------------------------------------------- G2
def test_plans_as_a_sweep(ctx, stock):
    """G2.  The two instances run different plans and offsets (cycle 80 / green 20 / amber 10 from tick 3; cycle 120 / 35 / 8 from tick 36):
    the same replay until everybody has arrived, arrivals those of the two CPU runs.  Instance 0 meets amber too close to its line to stop
    and drives on; instance 1 is held at amber (held = 2) and stays held through it."""
    sim = _straight(ctx, stock, plans=SWEEP, plan_of=np.array([0, 1]), offset=np.array(SWEEP_OFFSET))
    cpu = [_cpu_arrivals(s, o) for s, o in zip(SWEEP, SWEEP_OFFSET)]
    arr, worst, held, cut, recs = _stepped(sim, 260)
    amber = [int(sum((r['held'].reshape(2, 4)[b] == 2).sum() for r in recs)) for b in (0, 1)]
    print('sweep: worst %.2e, arrivals %s, held at amber per instance %s, amber passed %s' % (worst, arr, amber, [c.amber_free for c in cpu]))
    assert arr[:4] == cpu[0].arrival and arr[4:] == cpu[1].arrival and min(arr) > 0 and arr[:4] != arr[4:]
    assert cpu[0].amber_free > 0 and amber[1] >= 8


# ---------------------------------------------------------------- G3
def _same(a, b, what, skip=('held', 'tick')):
    assert sorted(k for k in a if k not in skip) == sorted(k for k in b if k not in skip), what
    for k in b:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_all_green_is_the_run_without_signals(ctx, stock, mode):
    """G3.  Every group green for the whole cycle: after every one of 40 steps every buffer equals that of a batch that never had signals,
    bit for bit; nobody is ever held and the clocks run"""
    a, b = _straight(ctx, stock, mode, plans=None), _straight(ctx, stock, mode, plans=None)
    a.signalise(dict(cycle=7, amber=0, green=np.array([[0, 7], [3, 7], [6, 7], [2, 7]])), offset=np.array([[0, 5, 9, -2], [1, 2, 3, 4]]))
    for s in range(40):
        a.run(1); b.run(1)
        x = _snap(a)
        _same(x, _snap(b), s)
        assert not x['held'].any()
    assert x['tick'].tolist() == [(t + 40) % 7 for t in (0, 5, 9, -2, 1, 2, 3, 4)]


def _entry(sim, signals, n, graph=0, **over):
    """mpcx_closed_loop_run_signals itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, retire=sim._retire, scene=sim._scene)
    st.update(over)
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_signals(c._ctx, C.byref(cip), C.byref(st['desc']), None, byref(sim._opts), byref(st['retire']), byref(st['scene']),
                                              byref(sim._admit), byref(sim._respawn), byref(sim._routes), byref(sim._precedence), byref(signals),
                                              int(n), int(graph)))


def test_off_means_off(ctx, stock):
    """G4.  signals = NULL and an all-zero struct through mpcx_closed_loop_run_signals, and unsignalise(), each give the bytes of a batch
    that never had signals: 40 steps of the straight scene"""
    from mpc_for_av_at_intersection_amd import _lib
    base = _straight(ctx, stock, plans=None)
    base.run(40)
    want = base.snapshot()
    runs = {}
    sim = _straight(ctx, stock, plans=None); _entry(sim, None, 40); runs['NULL'] = sim
    sim = _straight(ctx, stock, plans=None); _entry(sim, _lib.SignalsC(), 40); runs['zero struct'] = sim
    sim = _straight(ctx, stock); sim.unsignalise(); sim.run(40); runs['unsignalise'] = sim
    for name, sim in runs.items():
        got = sim.snapshot()
        assert 'held' not in got
        _same(got, want, name, skip=())
    assert not runs['unsignalise'].held.any() and not runs['unsignalise'].tick.any()        # no longer read or written
    held = _straight(ctx, stock); held.run(40)
    assert held.snapshot()['held'].tolist() == [0, 1, 0, 1] * 2 and held.snapshot()['state'].tobytes() != want['state'].tobytes()


# ---------------------------------------------------------------- G5
def test_graph_replay_in_chunks(ctx, stock):
    """G5.  The straight scene under the plan as 15 chunks of run(7, graph=True) on a side stream equals 105 x run(1) plain, byte for byte,
    tick and held included: the clock lives in device memory, so the one captured step keeps counting"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _straight(ctx, stock, offset=np.array([0, 50]))
    helds = set()
    for _ in range(105):
        plain.run(1)
        helds.add(tuple(plain.held.cpu().numpy().tolist()))
    a = _snap(plain)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _straight(side, stock, offset=np.array([0, 50]))
        torch.cuda.synchronize()
        for _ in range(15):
            graph.run(7, graph=True)
        b = _snap(graph)
        _same(a, b, 'graph', skip=())
        assert a['tick'].tolist() == [5] * 4 + [55] * 4 and len(helds) == 2 and a['done'].any()       # (held through the first half cycle, then free)
    finally:
        side.close()


# ---------------------------------------------------------------- G6
@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_host_staging_equals_the_loop(ctx, stock, mode):
    """G6.  step_staged() -- the per-stage entry points with mpcx_signal_step_batch between the conflict search and the window stage --
    equals run(1) after every one of 40 steps, tick and held included, on the plain loop without retirement; agents are held meanwhile"""
    X, Y = (_straight(ctx, stock, mode, offset=np.array([0, 50]), retire=False) for _ in range(2))
    held = np.zeros(8, dtype=np.int64)
    for s in range(40):
        X.run(1); Y.step_staged()
        x = _snap(X)
        _same(x, _snap(Y), s, skip=())
        held += x['held'] != 0
    # the phase that starts at red is held from the first step on (in cut mode it still stands at its line after 40 steps)
    assert (held[[1, 3, 4, 6]] > 10).all() and not held[[0, 2, 5, 7]].any() and 'done' not in x
    if mode == 'cut':
        assert x['held'].tolist() == [0, 1, 0, 1, 1, 0, 1, 0]


# ---------------------------------------------------------------- G7
def test_routed_respawn_batch_follows_the_host_rule(ctx, stock, ref):
    """G7.  The routed respawn batch of tests/test_gpu_route.py (two arms x two slots, G = 3; B = 2) under a short two-phase plan (cycle 40,
    green 12, amber 4), 150 steps.  After every step held, tick and cut_len equal the host build of the rule applied to the device's own
    words of that step: traj_idx as the step left it, the state before the step, the tables, and for the cut the conflict search's own
    (the path length where it found no conflict; where it found one the rule can only have lowered it, which is checked as such).  An agent
    that arrives is past its line and free; a vehicle that enters after a respawn enters with held = 0; routes did change under way."""
    from mpc_for_av_at_intersection_amd.batch import stop_lines
    sim = TR._routed(ctx, stock)
    stop, group = stop_lines(stock[0], setback=1.0)         # (the batch starts 3 m before the crossing: a line between start and crossing)
    sim.signalise(_plans(dict(cycle=40, green=12, amber=4))[0], stop=stop, group=group, offset=np.array([0, 7]))
    tabs = _tables(sim)
    seen, entered, lowered = set(), 0, 0
    offs0 = sim.path_off.cpu().numpy().copy()
    for s in range(150):
        before = _snap(sim)
        b_off, b_len = sim.path_off.cpu().numpy().copy(), sim.path_len.cpu().numpy().copy()
        sim.run(1)
        after = _snap(sim)
        admitted = (before['entered_step'] < 0) & (after['entered_step'] >= 0)
        assert not before['held'][admitted].any(), s
        entered += int((admitted & (before['served'] > 0)).sum())
        driving = (before['done'] == 0) | admitted
        arrived = driving & (after['done'] != 0)              # (respawn may have reset this slot's words already)
        keep = driving & ~arrived
        cut_in = np.where(after['hit_idx'] >= 0, after['cut_len'], b_len).astype(np.int32)
        w = G.words(state=before['state'], path_off=b_off, path_len=b_len, traj_idx=after['traj_idx'], cut_len=cut_in,
                    done=(~driving).astype(np.int32), tick=before['tick'], held=before['held'], dl=sim.dl, **tabs)
        G.host_rule(ref, w)
        assert np.array_equal(w['tick'], after['tick']), s
        assert np.array_equal(w['held'][~arrived], after['held'][~arrived]) and not after['held'][arrived].any(), (s, w['held'], after['held'])
        assert np.array_equal(w['cut_len'][keep], after['cut_len'][keep]), (s, w['cut_len'], after['cut_len'])
        hk = keep & (after['held'] != 0)
        line = tabs['path_stop'][(b_off + after['traj_idx'])[hk]]
        assert (after['cut_len'][hk] <= line).all() and (after['traj_idx'][hk] < line).all(), s
        lowered += int((after['cut_len'][hk] == line).sum())
        seen |= set(after['held'].tolist())
    print('routed respawn: held values seen %s, %d agent-steps cut at the line, %d respawned vehicles entered, %d episodes' %
          (sorted(seen), lowered, entered, len(sim.episodes())))
    assert seen >= {0, 1} and lowered > 20 and entered >= 2
    assert (sim.path_off.cpu().numpy() != offs0).any() and len(sim.episodes()) >= 4


# ---------------------------------------------------------------- G8
def test_signals_with_right_of_way(ctx, stock):
    """G8.  Signals together with give_way('entry') (admission on, everybody due at once) run to completion: everybody arrives, the two
    phases at the steps of the run with signals alone or later, and nobody is held at the end"""
    sim = _straight(ctx, stock, plans=None)
    sim.enter_on_schedule(np.zeros((2, 4), dtype=np.int64), gap=1.0)
    sim.give_way('entry')
    sim.signalise(_plans(G.PLAN)[0])
    taken = sim.run_until_done(400, chunk=20)
    snap = sim.snapshot()
    print('signals + first come first served: done after %d steps, steps driven %s' % (taken, snap['steps_driven'].tolist()))
    assert snap['done'].all() and snap['absent'].all() and not snap['held'].any() and 'precedence' in snap
    assert (snap['steps_driven'].reshape(2, 4)[:, [1, 3]] >= 98).all() and taken <= 400


# ---------------------------------------------------------------- G9
def test_refusals(ctx, stock):
    """G9.  MPCX_E_INVALID with a "signals: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: a NULL pointer, n_groups outside 1..16, n_plans < 1, n_points < 1, a brake that is not finite or not positive,
    cycle < 1, amber < 0, green_from outside [0, cycle), green_len < 0, green_len + amber > cycle, the agent-sharded layout, more than one
    linearisation pass; the stage-level call refuses the same way.  In Python: malformed plans and tables."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _straight(ctx, stock)
    before = _snap(sim)
    sg = sim._signals
    names = [n for n, _ in _lib.SignalsC._fields_]
    good = {n: getattr(sg, n) for n in names}
    make = lambda **kw: _lib.SignalsC(**dict(good, **kw))

    def refused(match, signals, **over):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _entry(sim, signals, n, graph, **over)
    for n in names[:8]:
        refused(r'mpcx error -1: signals: .*%s is null' % n, make(**{n: None}))
    for n in (0, -1, 17):
        refused(r'mpcx error -1: signals: n_groups = %d outside 1\.\.16' % n, make(n_groups=n))
    refused(r'mpcx error -1: signals: n_plans = 0', make(n_plans=0))
    refused(r'mpcx error -1: signals: n_points = 0', make(n_points=0))
    for b in (0.0, -1.0, float('inf'), float('nan')):
        refused(r'mpcx error -1: signals: brake', make(brake=b))

    def plan(cycle=100, amber=8, green=((0, 30), (50, 30), (0, 30), (50, 30))):
        t = (ctx.i32(np.array([cycle])), ctx.i32(np.array([amber])), ctx.i32(np.array([green])))
        ctx.synchronize()
        return t, make(plan_cycle=t[0].data_ptr(), plan_amber=t[1].data_ptr(), plan_green=t[2].data_ptr())
    for kw, match in ((dict(cycle=0), 'cycle = 0'), (dict(amber=-1), 'amber = -1'),
                      (dict(green=((0, 30), (100, 30), (0, 30), (50, 30))), r'group 1 has green_from = 100 outside \[0, 100\)'),
                      (dict(green=((-1, 30), (50, 30), (0, 30), (50, 30))), 'group 0 has green_from = -1'),
                      (dict(green=((0, 30), (50, 30), (0, -2), (50, 30))), 'group 2 has green_len = -2'),
                      (dict(green=((0, 30), (50, 30), (0, 30), (50, 93))), r'group 3 has green_len \+ amber = 93 \+ 8 > cycle = 100')):
        keep, bad = plan(**kw)
        refused(r'mpcx error -1: signals: plan 0 ' + match if 'group' in match else r'mpcx error -1: signals: plan 0 has ' + match, bad)
    keep, fine = plan(green=((0, 92), (99, 0), (0, 0), (50, 30)))       # the limits themselves are accepted
    _entry(sim, fine, 0)
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 2, 4, sim.obs6.data_ptr()
    refused(r'mpcx error -1: signals: not supported in the agent-sharded layout', sg, desc=shard, retire=None, scene=None)
    ctx.set_linearisation_passes(2)
    try:
        sim.lin_passes = 2
        refused(r'mpcx error -1: signals: 2 linearisation passes', sg, retire=None, scene=None)
        with pytest.raises(MpcxError, match='signals: 2 linearisation passes'):
            ctx.signal_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sg)
    finally:
        sim.lin_passes = 1
        ctx.set_linearisation_passes(1)
    # the stage-level call refuses the same way, before its launch
    for bad, match in ((make(held=None), 'held is null'), (make(n_groups=40), 'n_groups = 40'), (make(brake=-2.0), 'brake'),
                       (plan(cycle=-3)[1], 'cycle = -3')):
        with pytest.raises(MpcxError, match='signals: .*' + match):
            ctx.signal_step(sim.dl, sim.state, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], bad, done=sim.done)
    ctx.synchronize()
    _same(_snap(sim), before, 'refused', skip=())
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any()
    # ---- Python
    pl = _plans(G.PLAN)[0]
    n = int(sim.path.shape[0])
    for kw in (dict(plans=[]), dict(plans=[pl, dict(pl, green=pl['green'][:2])]), dict(plans=dict(pl, green=np.zeros((17, 2), dtype=np.int64))),
               dict(plans=pl, stop=np.zeros(n, dtype=np.int32)), dict(plans=pl, stop=np.zeros(3, dtype=np.int32), group=np.zeros(3, dtype=np.int32)),
               dict(plans=pl, plan_of=np.zeros(3, dtype=np.int64)), dict(plans=pl, offset=np.zeros((2, 4)))):
        with pytest.raises(ValueError):
            sim.signalise(**kw)
    assert sim._signals is sg
    sim.unsignalise()
    assert sim._signals is None and 'held' not in sim.snapshot()
