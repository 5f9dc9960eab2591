"""GPU tests of SIGNAL-AWARE APPROACH SPEED in the device-resident closed loop (mpcx_closed_loop_run_advised, IntersectionBatch.advise_speed):
one launch between the window stage and the QP caps the speed reference of an agent that would reach its stop line on red at the speed
with which it reaches the line as the light turns green.  The defining property: every driving agent of every step equals the oracle step
in which the speed profile is replaced by its minimum with the advised speed (advise_helpers.advise_agent_step), and `advised` equals the
host build of the rule bit for bit -- on the scene tests/test_advise_cpu.py pins on the CPU oracle alone.  Then: the rule on a routed
respawn batch, off means off, graph replay, host staging, the refusals.  B = 2, A = 4, T = 13, v0 = 0, speed mode."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import advise_helpers as AH
from tests import scene_helpers as SH
from tests import signal_helpers as G
from tests import test_gpu_route as TR
from tests import test_gpu_scene as GS
from tests import test_gpu_signal as TS

pytestmark = pytest.mark.gpu

KEYS = GS.KEYS
OFFSET = np.array([60, 75])         # the clocks of the two instances: 40 and 25 steps of red left for the first phase


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
    return AH.build_ref(tmp_path_factory.mktemp('advise_ref'))


def _advised(c, stock, advise=True, offset=OFFSET, retire=True, plans=(G.PLAN,)):
    """B = 2 instances of the four straight routes from index 0 in speed mode under signals, with advice unless told otherwise"""
    sim = TS._straight(c, stock, 'speed', plans=plans, offset=offset, retire=retire)
    if advise:
        sim.advise_speed()
    return sim


def _params(sim):
    a = sim._advice
    return dict(v_cruise=float(a.v_cruise), v_min=float(a.v_min), reach=float(a.reach), lead=int(a.lead))


def _host_words(sim, tabs, traj_idx, cut_len, tick, done, xref, path_off=None, path_len=None):
    """the device's own words of a step as the host build takes them"""
    t = {k: tabs[k] for k in ('path_stop', 'path_group', 'plan_cycle', 'plan_amber', 'plan_green', 'plan_of')}
    return AH.words(path_off=sim.path_off.cpu().numpy() if path_off is None else path_off,
                    path_len=sim.path_len.cpu().numpy() if path_len is None else path_len, traj_idx=traj_idx, cut_len=cut_len, tick=tick, done=done,
                    xref=xref, dl=sim.dl, dt=float(sim.params.dt), **t, **_params(sim))


def _replay_step(sim, ref, before, after, pool, absent, tabs):
    """Every DRIVING agent of the step replayed on the oracle with both rules (advise_helpers.advise_agent_step).  traj_idx, the stop index,
    hit_idx, target_ind, status, held, done and absent identical; advised equal to the host build applied to the device's words, bitwise,
    and to the oracle's; row 2 of xref equal to the oracle's capped profile; u and x within 2e-7 (the project's bar).  A retired agent's
    buffers are unchanged and it is not advised.  Returns (worst difference, agents advised, agents whose window the cap lowered)."""
    from oracle import oracle_py as orc
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    stop = sim.stop_index()
    adv = _params(sim)
    w = _host_words(sim, tabs, after['traj_idx'], after['cut_len'], after['tick'], before['done'], np.zeros_like(after['xref']))
    AH.host_rule(ref, w)
    assert w['advised'].tobytes() == after['advised'].tobytes(), (w['advised'], after['advised'])
    worst, n_adv, n_low = 0.0, 0, 0
    for p in range(sim.P):
        plan = int(tabs['plan_of'][p])
        cycle = int(tabs['plan_cycle'][plan])
        t = int(before['tick'][p]) % cycle
        assert after['tick'][p] == (t + 1) % cycle, p
        if before['done'][p]:
            for k in KEYS:
                if k != 'applied':
                    assert before[k][p].tobytes() == after[k][p].tobytes(), (p, k)
            assert not after['applied'][p].any() and after['held'][p] == 0 and after['advised'][p] == 0.0
            continue
        present = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p] and not absent[r]]

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

        def advise(ti, cut, p=p, plan=plan, cycle=cycle, t=t):
            s, g = line(ti)
            if s < 0 or ti >= s or s >= ln[p] or cut < s:
                return 0.0
            return AH.advised_speed(ti, s, (t + 1) % cycle, cycle, int(tabs['plan_green'][plan, g, 0]), int(tabs['plan_green'][plan, g, 1]), sim.dl,
                                    float(sim.params.dt), **adv)
        r = AH.advise_agent_step(po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], pool[present], int(before['traj_idx'][p]),
                                 int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                                 sim.ip.cutoff_margin, decide, advise, v_ref=sim.v_ref)
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        want = (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status, r['held'])
        got = (after['traj_idx'][p], stop[p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p])
        assert want == tuple(int(v) for v in got), (p, want, got)
        assert after['cut_len'][p] == (r['cut'] if (r['hit'] is not None or r['held']) else ln[p]), p
        assert r['sol'].status == 0
        assert np.float64(r['advised']).tobytes() == after['advised'][p].tobytes(), (p, r['advised'], after['advised'][p])
        assert np.array_equal(np.asarray(r['xref'])[2], after['xref'][p, 2]), (p, r['xref'][2], after['xref'][p, 2])
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        n_adv += r['advised'] > 0.0
        n_low += bool((np.asarray(r['xref'])[2] < np.asarray(r['xref_free'])[2]).any())
        arrived = SH.is_goal(after['state'][p], tab[off[p] + ln[p] - 1], after['target_ind'][p], ln[p])
        assert bool(after['done'][p]) == arrived and after['absent'][o_skip[p]] == int(arrived), (p, arrived)
    assert worst < 2e-7, worst
    return worst, n_adv, n_low


# ---------------------------------------------------------------- G1
def test_straight_scene_on_the_oracle(ctx, stock, ref):
    """G1.  tests/test_advise_cpu.py's scene (four straight routes from index 0 in speed mode under signal_helpers.PLAN, departure on); the
    two instances start at clocks 60 and 75.  After every step until all have arrived every driving agent equals the AdviceOracleLoop
    step, `advised` equals the host build bitwise, and both instances arrive at the steps of the CPU oracle's own runs.  Not vacuous:
    agents are advised, and the cap lowered entries of their windows."""
    sim = _advised(ctx, stock)
    cpu = [AH.straight_loop(int(o)) for o in OFFSET]
    for c in cpu:
        c.run(600)
    tabs = TS._tables(sim)
    worst, n_adv, n_low, arr = 0.0, 0, 0, np.full(sim.P, -1)
    for s in range(260):
        before = TS._snap(sim)
        sim.run(1)
        after = TS._snap(sim)
        w, a, l = _replay_step(sim, ref, before, after, GS._pool_before(sim, before, after), before['absent'], tabs)
        worst, n_adv, n_low = max(worst, w), n_adv + a, n_low + l
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        if after['done'].all():
            break
    arr = arr.tolist()
    print('worst |GPU - oracle| %.2e over %d steps, arrivals %s, %d agent-steps advised, %d windows lowered' % (worst, s + 1, arr, n_adv, n_low))
    assert arr[:4] == cpu[0].arrival and arr[4:] == cpu[1].arrival and min(arr) > 0
    assert arr == [99, 59, 99, 59, 71, 107, 71, 107]
    assert n_adv > 30 and n_low > 30 and after['absent'].all() and not after['advised'].any()


# ---------------------------------------------------------------- G2
def test_routed_respawn_batch_follows_the_host_rule(ctx, stock, ref):
    """G2.  The routed respawn batch of tests/test_gpu_route.py (two arms x two slots, G = 3; B = 2) in speed mode under a short two-phase
    plan (cycle 40, green 12, amber 4), 60 steps.  After every step `advised` and row 2 of xref equal the host build of the rule applied to
    the device's own words of that step, bitwise: traj_idx, the stop index and the clock as the step left them, the route the agent was
    on, and a window whose entries -- the speed profile holds v_ref or 0 -- are v_ref wherever the device's are not 0.  (A slot that
    arrives is reset by the respawn stage behind the advice: its words are no longer those of the step.)"""
    from mpc_for_av_at_intersection_amd.batch import stop_lines
    sim = TR._routed(ctx, stock, 'speed')
    stop, group = stop_lines(stock[0], setback=1.0)         # (the batch starts 3 m before the crossing: a line between start and crossing)
    sim.signalise(TS._plans(dict(cycle=40, green=12, amber=4))[0], stop=stop, group=group, offset=np.array([0, 7]))
    sim.advise_speed(reach=30.0)
    tabs = TS._tables(sim)
    n_adv, n_low, seen = 0, 0, 0
    for s in range(60):
        before = TS._snap(sim)
        b_off, b_len = sim.path_off.cpu().numpy().copy(), sim.path_len.cpu().numpy().copy()
        sim.run(1)
        after = TS._snap(sim)
        admitted = (before['entered_step'] < 0) & (after['entered_step'] >= 0)
        driving = (before['done'] == 0) | admitted
        keep = driving & (after['done'] == 0)
        row2 = after['xref'][:, 2]
        assert ((row2 == 0.0) | (row2 == sim.v_ref) | (row2 == after['advised'][:, None]))[keep].all(), s
        free = np.zeros_like(after['xref'])
        free[:, 2] = np.where(row2 != 0.0, sim.v_ref, 0.0)
        w = _host_words(sim, tabs, after['traj_idx'], after['cut_len'], after['tick'], (~driving).astype(np.int32), free.copy(), b_off, b_len)
        AH.host_rule(ref, w)
        assert w['advised'][keep].tobytes() == after['advised'][keep].tobytes(), (s, w['advised'], after['advised'])
        assert w['xref'][keep, 2].tobytes() == row2[keep].tobytes(), s
        assert not after['advised'][~driving].any(), s
        n_adv += int((after['advised'][keep] > 0).sum())
        n_low += int((w['xref'][keep, 2] < free[keep, 2]).any(axis=1).sum())
        seen += int(keep.sum())
    print('routed respawn: %d of %d agent-steps advised, %d windows lowered' % (n_adv, seen, n_low))
    assert n_adv > 10 and n_low > 10 and seen > n_adv


# ---------------------------------------------------------------- G3
def _entry(sim, advice, n, graph=0, **over):
    """mpcx_closed_loop_run_advised itself, with the structs of `sim` unless given"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    st = dict(desc=sim._desc, opts=sim._opts, retire=sim._retire, scene=sim._scene, signals=sim._signals, actuation=sim._actuation)
    st.update(over)
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_advised(c._ctx, C.byref(cip), C.byref(st['desc']), None, byref(st['opts']), byref(st['retire']),
                                              byref(st['scene']), byref(sim._admit), byref(sim._respawn), byref(sim._routes),
                                              byref(sim._precedence), byref(st['signals']), byref(st['actuation']), byref(advice), int(n), int(graph)))


def test_off_means_off(ctx, stock):
    """G3.  advice = NULL and an all-zero struct through mpcx_closed_loop_run_advised, and stop_advising(), each give the bytes of a batch
    that never had advice: 40 steps of the straight scene, in which the batch with advice does differ.  Under an all-green plan nobody is
    ever advised and every buffer equals that of the batch without advice after every step."""
    from mpc_for_av_at_intersection_amd import _lib
    base = _advised(ctx, stock, advise=False)
    base.run(40)
    want = TS._snap(base)
    runs = {}
    sim = _advised(ctx, stock, advise=False); _entry(sim, None, 40); runs['NULL'] = sim
    sim = _advised(ctx, stock, advise=False); _entry(sim, _lib.AdviceC(), 40); runs['zero struct'] = sim
    sim = _advised(ctx, stock); sim.stop_advising(); sim.run(40); runs['stop_advising'] = sim
    for name, sim in runs.items():
        got = TS._snap(sim)
        assert 'advised' not in got
        TS._same(got, want, name, skip=())
    assert not runs['stop_advising'].advised.any()          # no longer written
    on = _advised(ctx, stock); on.run(40)
    got = TS._snap(on)
    assert (got['advised'] > 0).any() and got['state'].tobytes() != want['state'].tobytes()
    on.unsignalise()
    assert on._advice is None and 'advised' not in on.snapshot()
    green = dict(cycle=7, amber=0, green=np.array([[0, 7], [3, 7], [6, 7], [2, 7]]))
    a, b = (TS._straight(ctx, stock, 'speed', plans=None) for _ in range(2))
    for sim in (a, b):
        sim.signalise(green, offset=np.array([[0, 5, 9, -2], [1, 2, 3, 4]]))
    a.advise_speed()
    for s in range(40):
        a.run(1); b.run(1)
        x = TS._snap(a)
        assert not x.pop('advised').any(), s
        TS._same(x, TS._snap(b), s, skip=())


# ---------------------------------------------------------------- G4
def test_graph_replay_in_chunks(ctx, stock):
    """G4.  The straight scene with advice as 15 chunks of run(7, graph=True) on a side stream equals 105 x run(1) plain, byte for byte,
    tick, held and advised included"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _advised(ctx, stock)
    n_adv = 0
    for _ in range(105):
        plain.run(1)
        n_adv += int((plain.advised > 0).sum())
    a = TS._snap(plain)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _advised(side, stock)
        torch.cuda.synchronize()
        for _ in range(15):
            graph.run(7, graph=True)
        b = TS._snap(graph)
        TS._same(a, b, 'graph', skip=())
        assert 'advised' in a and n_adv > 30 and a['done'].any()
    finally:
        side.close()


# ---------------------------------------------------------------- G5
def test_host_staging_equals_the_loop(ctx, stock):
    """G5.  step_staged() -- the per-stage entry points with mpcx_advise_step_batch between the window stage and the QP -- equals run(1)
    after every one of 40 steps, advised included, on the plain loop without retirement; agents are advised meanwhile"""
    X, Y = (_advised(ctx, stock, retire=False) for _ in range(2))
    n_adv = np.zeros(8, dtype=np.int64)
    for s in range(40):
        X.run(1); Y.step_staged()
        x = TS._snap(X)
        TS._same(x, TS._snap(Y), s, skip=())
        n_adv += x['advised'] > 0
    assert n_adv.sum() > 30 and (n_adv > 0).sum() >= 4 and 'done' not in x


# ---------------------------------------------------------------- G6
def test_refusals(ctx, stock):
    """G6.  MPCX_E_INVALID with an "advice: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: advised NULL, n_rows != P, v_cruise / v_min / reach not finite or not positive, v_min > v_cruise, lead < 0, no
    signals, actuation on, a stop mode other than MPCX_STOP_SPEED.  The stage call refuses the same way before its launch (it has no
    actuation and no stop mode to look at: signals without a plan, which is what actuation leaves, are refused there).  In Python:
    advise_speed() outside speed mode, without signalise(), with malformed values."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _advised(ctx, stock)
    before = TS._snap(sim)
    ad = sim._advice
    names = [n for n, _ in _lib.AdviceC._fields_]
    good = {n: getattr(ad, n) for n in names}
    make = lambda **kw: _lib.AdviceC(**dict(good, **kw))
    xref = sim.pre['xref']

    def stage(advice, signals=None):
        ctx.advise_step(sim.dl, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sim._signals if signals is None else signals,
                        advice, xref, done=sim.done)

    def refused(match, advice, staged=True, **over):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _entry(sim, advice, n, graph, **over)
        if staged:
            with pytest.raises(MpcxError, match=match):
                stage(advice, over.get('signals'))
    refused(r'mpcx error -1: advice: advised is null', make(advised=None))
    for n in (0, 7, 9, -8):
        refused(r'mpcx error -1: advice: n_rows = %d is not P = 8' % n, make(n_rows=n))
    for name in ('v_cruise', 'v_min', 'reach'):
        for v in (0.0, -1.0, float('inf'), float('nan')):
            refused(r'mpcx error -1: advice: %s = .* must be finite and positive' % name, make(**{name: v}))
    refused(r'mpcx error -1: advice: v_min = 7 > v_cruise = 6', make(v_min=7.0, v_cruise=6.0))
    refused(r'mpcx error -1: advice: lead = -1 is negative', make(lead=-1))
    _entry(sim, make(v_min=good['v_cruise'], lead=0), 0)        # the limits themselves are accepted
    # no signals: through the loop NULL and the all-zero struct, through the stage call the all-zero struct
    refused(r'mpcx error -1: advice: needs signals', ad, staged=False, signals=None)
    refused(r'mpcx error -1: advice: needs signals', ad, signals=_lib.SignalsC())
    # the signals' own refusals come through
    sg = sim._signals
    bad = _lib.SignalsC(**dict({n: getattr(sg, n) for n, _ in _lib.SignalsC._fields_}, brake=-1.0))
    refused(r'mpcx error -1: signals: brake', ad, signals=bad)
    # actuation on
    act = _advised(ctx, stock, advise=False)
    act.actuate(two_phase_controller(min_green=5, max_green=30, gap=3, amber=4, all_red=2, detect=60))
    refused(r'mpcx error -1: advice: not with actuation', ad, staged=False, signals=act._signals, actuation=act._actuation)
    with pytest.raises(MpcxError, match='advice: the signals carry no fixed plan'):
        stage(ad, act._signals)
    # cut mode
    cut = TS._straight(ctx, stock, 'cut', offset=OFFSET)
    cut_before = TS._snap(cut)
    for graph in (0, 1):
        for n in (0, 1):
            with pytest.raises(MpcxError, match='mpcx error -1: advice: the stop mode is not MPCX_STOP_SPEED'):
                _entry(cut, ad, n, graph)
    ctx.synchronize()
    TS._same(TS._snap(sim), before, 'refused', skip=())
    TS._same(TS._snap(cut), cut_before, 'refused in cut mode', skip=())
    assert sim.steps_done == 0 and not sim.steps_driven.any() and not sim.absent.any() and not sim.advised.any()
    assert not act.junction_state.any() and not act.held.any()
    # ---- Python
    with pytest.raises(ValueError, match='stop_mode'):
        cut.advise_speed()
    with pytest.raises(ValueError, match='signalise'):
        TS._straight(ctx, stock, 'speed', plans=None).advise_speed()
    with pytest.raises(ValueError, match='signalise'):
        act.advise_speed()
    for kw in (dict(v_min=0.0), dict(v_min=9.0), dict(reach=-1.0), dict(lead=-1), dict(v_cruise=float('nan')), dict(reach=float('inf'))):
        with pytest.raises(ValueError):
            sim.advise_speed(**kw)
    assert sim._advice is ad
    sim.stop_advising()
    assert sim._advice is None and 'advised' not in sim.snapshot() and 'held' in sim.snapshot()
