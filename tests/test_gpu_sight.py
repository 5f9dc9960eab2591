"""Line of sight on the device (mpcx_sight, csrc/mpcx_sight.hip, csrc/mpcx_interaction_sight.hip): the stage call against the host build of
the rule byte for byte; inside the closed loop every driving agent of every step against the oracle step over the rows its sight word
leaves it (sight_helpers.SightOracleLoop's filter), alone and with right of way on top; off means off; graph replay; the near-miss log
keeps seeing the physical scene; the refusals."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import precedence_helpers as PH
from tests import scene_helpers as SH
from tests import sight_helpers as ST
from tests import test_gpu_precedence as GP
from tests import test_gpu_scene as GS

pytestmark = pytest.mark.gpu


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
    return ST.build_ref(tmp_path_factory.mktemp('sight_ref'))


def _device_step(c, w):
    """the stage call on the words of sight_helpers: (sight uint64, n_seen, n_hidden) and the struct"""
    from mpc_for_av_at_intersection_amd import _lib
    w = ST.tidy(w)
    dev = c.device
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {k: up(w[k]) for k in ('state', 'obs6', 'obs_off', 'obs_cnt', 'obs_skip', 'set_of', 'done', 'absent', 'heard', 'hp_off', 'set_off')}
    t['hp'], t['box'] = up(w['hp'].reshape(-1)), up(w['box'].reshape(-1))
    P = w['P']
    sight = torch.full((P,), 0x5555, dtype=torch.int64, device=dev)
    seen, hidden = torch.full((P,), -7, dtype=torch.int32, device=dev), torch.full((P,), -7, dtype=torch.int32, device=dev)
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    s = _lib.SightC(ptr(sight), ptr(seen), ptr(hidden), ptr(t['hp']), ptr(t['hp_off']), ptr(t['box']), ptr(t['set_off']), ptr(t['set_of']),
                    ptr(t['heard']), w['range'], len(w['hp_off']) - 1, len(w['set_off']) - 1, P, w['n_pool'], 0)
    c.sight_step(t['state'], t['obs6'], t['obs_off'], t['obs_cnt'], t['obs_skip'], s, done=t['done'], absent=t['absent'])
    c.synchronize()
    return sight.cpu().numpy().view(np.uint64), seen.cpu().numpy(), hidden.cpu().numpy()


def test_stage_call_equals_the_host_build(ctx, ref):
    """V1.  mpcx_sight_step_batch on the hand-made words (the probes, the windows of 1 .. 70 rows with and without the scene's words, the
    shrunk square) equals the values written down by hand, and on 12 seeded scenes of P = 5, 17, 33 the host build, byte for byte"""
    for w, exp in ST.probe_words() + list(ST.window_words()) + [ST.shrunk_probe()]:
        ST.same(_device_step(ctx, w), exp, 'device vs by hand')
    sizes = set()
    for seed in range(12):
        w = ST.random_words(seed)
        got = _device_step(ctx, w)
        ST.same(got, ST.host_step(ref, w), 'seed %d: device vs host' % seed)
        assert got[1].sum() > 0 and got[2].sum() > 0
        sizes.add(len(w['state']))
    assert sizes == {5, 17, 33}


# ---------------------------------------------------------------- inside the loop
def _blind(c, stock, order=None, entry=False, occlude=True, **kw):
    """B = 2 instances of the four straight routes from index 0 (T = 13): corner_blocks() in instance 0, the empty set in instance 1; the
    range is 100 m (the cars of opposite arms start 60.3 m apart)"""
    from mpc_for_av_at_intersection_amd.batch import corner_blocks
    kw.setdefault('sensor_range', 100.0)
    sim = GP._straight(c, stock, order=order)
    if entry:
        sim.enter_on_schedule(np.array([[0, 3, 0, 5], [6, 0, 2, 0]]), gap=1.0)
        sim.give_way('entry')
    if occlude:
        sim.occlude([corner_blocks(), []], set_of=np.array([0, 1]), **kw)
    return sim


def _host_words(sim, before, after, pool, ref):
    """the sight words of the step before -> after through the host build, from the states before the step and the retirement and scene
    words as the head of the step (admission) left them"""
    t = sim._sight_tabs
    done, absent = before['done'] & after['done'], before['absent'] & after['absent']
    w = dict(state=before['state'], obs6=pool, obs_off=sim.obs_off.cpu().numpy(), obs_cnt=sim.obs_cnt.cpu().numpy(),
             obs_skip=sim.obs_skip.cpu().numpy(), set_of=t[4].cpu().numpy(), done=done, absent=absent,
             heard=None if t[5] is None else t[5].cpu().numpy(), hp=t[0].cpu().numpy(), hp_off=t[1].cpu().numpy(), box=t[2].cpu().numpy(),
             set_off=t[3].cpu().numpy(), range=sim._sight.range)
    return ST.host_step(ref, w), done, absent


def _replay_step(sim, before, after, ref):
    """every DRIVING agent of the step replayed on the oracle with the obstacle list = its pool window minus its own row minus the absent
    rows minus the rows its sight word hides (SightOracleLoop's filter), the yielding ones standing where there is right of way.  The
    sight words are the host build's, byte for byte; hit_idx, cut_len, traj_idx, target_ind and status identical, u and x within 2e-7.
    Returns (worst difference, agent-steps in which the unfiltered list gives another conflict, hidden candidates)."""
    from oracle import oracle_py as orc
    pool = GS._pool_before(sim, before, after)
    want, done, absent = _host_words(sim, before, after, pool, ref)
    ST.same((after['sight'], after['n_seen'], after['n_hidden']), want, 'sight words')
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    prec = after['precedence'] if 'precedence' in after else None
    worst, differs = 0.0, 0
    for p in range(sim.P):
        if done[p]:
            for k in ('traj_idx', 'target_ind', 'hit_idx', 'cut_len', 'status', 'u', 'x'):
                assert before[k][p].tobytes() == after[k][p].tobytes(), (p, k)
            assert int(after['sight'][p]) == 0
            continue
        everybody = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p] and not absent[r]]
        present = [r for r in everybody if (int(after['sight'][p]) >> (r - o_off[p])) & 1]
        view = (lambda rows: pool[rows]) if prec is None else (lambda rows: PH.view(pool, rows, prec[o_skip[p]], prec))
        step = lambda rows: orc.agent_step(po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], view(rows), int(before['traj_idx'][p]),
                                           int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                                           sim.ip.cutoff_margin)
        r = step(present)
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p])
        assert (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status) == got, (p, r['traj_idx'], r['cut'], want_hit, got)
        assert r['sol'].status == 0
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        if len(present) < len(everybody):
            differs += (step(everybody)['hit'] is None) != (r['hit'] is None)
    assert worst < 2e-7, worst
    return worst, differs, int(after['n_hidden'].sum())


@pytest.mark.parametrize('rule', ['none', 'fixed', 'entry'])
def test_loop_on_the_oracle(ctx, stock, ref, rule):
    """V2.  B = 2, A = 4, T = 13, 40 steps of run(1), corner blocks on instance 0 and the empty set on instance 1: after every step the sight
    words are the host build's and every driving agent equals the oracle step over the rows it sees -- without right of way, with a fixed
    order and with give_way('entry') behind an entry schedule.  Not vacuous: rows were hidden, in instance 0 only, and there are agent-steps
    in which the whole list would have given another conflict (so a conflict search without the AND fails here)."""
    sim = _blind(ctx, stock, order=((0, 1, 2, 3), (3, 2, 1, 0)) if rule == 'fixed' else None, entry=rule == 'entry')
    worst, differs, hidden0, hidden1 = 0.0, 0, 0, 0
    for s in range(40):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        w, d, _ = _replay_step(sim, before, after, ref)
        worst, differs = max(worst, w), differs + d
        hidden0, hidden1 = hidden0 + int(after['n_hidden'][:4].sum()), hidden1 + int(after['n_hidden'][4:].sum())
    print('%s: worst |GPU - oracle| %.2e, %d hidden agent-rows in the blind instance, %d changed conflicts' % (rule, worst, hidden0, differs))
    assert hidden0 > 40 and hidden1 == 0 and differs > 0


def _same(a, b, what, skip=()):
    assert sorted(k for k in a if k not in skip) == sorted(k for k in b if k not in skip), what
    for k in b:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


WORDS = ('sight', 'n_seen', 'n_hidden')


def test_empty_sets_and_off_mean_the_plain_run(ctx, stock):
    """V3.  With the empty set everywhere (and the range beyond every pair) the run equals the run without the stage on every snapshot()
    buffer and on the run log -- rows() and outcomes(), the per-step clearance column included --, byte for byte; NULL
    (see_everything()), an all-zero struct and a batch that never had the stage give the same bytes too, 40 steps.  With the corner blocks
    the run differs, and the log's clearance of every step is still the physical one."""
    from mpc_for_av_at_intersection_amd import _lib

    def same_log(log, what):
        assert log.rows().tobytes() == want_rows.tobytes(), what
        o = log.outcomes()
        assert sorted(o) == sorted(want_out) and all(o[k].tobytes() == want_out[k].tobytes() for k in o), what
    plain = _blind(ctx, stock, occlude=False)
    plain_log = plain.attach_log(40)
    plain.run(40)
    want, want_rows, want_out = plain.snapshot(), plain_log.rows(), plain_log.outcomes()
    assert want_rows.shape == (40, plain.P) and np.isfinite(want_rows['clearance']).all()
    empty = _blind(ctx, stock, occlude=False)
    empty_log = empty.attach_log(40)
    empty.occlude([], sensor_range=float('inf'))
    empty.run(40)
    got = empty.snapshot()
    assert (got['n_hidden'] == 0).all() and got['n_seen'].sum() > 0
    _same(got, want, 'empty set', skip=WORDS)
    same_log(empty_log, 'empty set')
    off = _blind(ctx, stock)
    off_log = off.attach_log(40)
    off.see_everything()
    off.run(40)
    _same(off.snapshot(), want, 'see_everything')
    same_log(off_log, 'see_everything')
    assert not off.sight.any().item()
    zero = _blind(ctx, stock, occlude=False)
    zero_log = zero.attach_log(40)
    zero._sight = _lib.SightC()
    zero.run(40)
    zero._sight = None
    _same(zero.snapshot(), want, 'zero struct')
    same_log(zero_log, 'zero struct')
    # corner blocks change what the agents do, not what the log measures: its clearance of a step is the physical one (the numpy
    # restatement over every present row, hidden or not; 1e-9, the run log's bar)
    blind = _blind(ctx, stock)
    blind_log = blind.attach_log(40)
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (blind.obs_off, blind.obs_cnt, blind.obs_skip))
    centers, truth = np.asarray(blind.ip.circle_centers).reshape(2, 2), []
    for s in range(40):
        before = blind.snapshot()
        blind.run(1)
        pool = GS._pool_before(blind, before, blind.snapshot())
        for p in range(blind.P):
            if not before['done'][p]:
                present = [x for x in range(o_off[p], o_off[p] + o_cnt[p]) if x != o_skip[p] and not before['absent'][x]]
                truth.append((p, SH.clearance(pool, o_skip[p], present, centers, blind.ip.radius) if present else np.inf))
    assert blind_log.rows().tobytes() != want_rows.tobytes(), 'the corner blocks change the run'
    for q in range(blind.P):
        mine, logged = np.array([c for p, c in truth if p == q]), blind_log.rows(q)['clearance']
        assert len(logged) == len(mine) > 0 and np.all((logged == mine) | (np.abs(logged - mine) < 1e-9)), q
    gone = _blind(ctx, stock)       # keep_driving() and retire_at_goal() drop it with the scene
    gone.keep_driving()
    assert gone._sight is None and gone._scene is None
    again = _blind(ctx, stock)
    again.retire_at_goal(leave_scene=True)
    assert again._sight is None and 'sight' not in again.snapshot()


def test_graph_replay_and_a_range_changed_in_place(ctx, stock):
    """V4.  5 chunks of run(7, graph=True) on a side stream equal 35 x run(1) plain, byte for byte, the sight words included; then the range
    is changed in place in the struct: the cached graph's key covers the struct by value, so the next chunk is captured again and equals
    the plain run with the same change (more rows are hidden at 12 m than at 60 m)"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _blind(ctx, stock)
    for _ in range(35):
        plain.run(1)
    a = plain.snapshot()
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _blind(side, stock)
        torch.cuda.synchronize()
        for _ in range(5):
            graph.run(7, graph=True)
        _same(graph.snapshot(), a, 'graph')
        assert a['sight'].any()
        for sim in (plain, graph):
            sim._sight.range = 12.0
        for _ in range(7):
            plain.run(1)
        graph.run(7, graph=True)
        b = plain.snapshot()
        _same(graph.snapshot(), b, 'graph after the change')
        assert b['n_hidden'][4:].sum() > 0, 'at 12 m even the open junction hides somebody'
    finally:
        side.close()


def test_the_near_miss_log_sees_a_hidden_partner(ctx, stock):
    """V5.  with watch_safety() on, the log's nearest vehicle is the physical one: in the blind instance there are agent-steps whose partner
    is a row the agent does not see, and near_clearance is the true clearance over every present row (the numpy restatement, 1e-9)"""
    sim = _blind(ctx, stock)
    sim.watch_safety()
    centers, hidden_partner = np.asarray(sim.ip.circle_centers).reshape(2, 2), 0
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    for s in range(30):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        pool = GS._pool_before(sim, before, after)
        for p in range(sim.P):
            if before['done'][p]:
                continue
            r = int(after['partner'][p])
            present = [x for x in range(o_off[p], o_off[p] + o_cnt[p]) if x != o_skip[p] and not before['absent'][x]]
            if not present:
                continue
            assert abs(after['near_clearance'][p] - SH.clearance(pool, o_skip[p], present, centers, sim.ip.radius)) < 1e-9, (s, p)
            hidden_partner += r >= 0 and not (int(after['sight'][p]) >> (r - o_off[p])) & 1
    assert hidden_partner > 10, hidden_partner


def test_refusals(ctx, stock):
    """V6.  MPCX_E_INVALID with a "sight: ..." message before anything is launched, whatever n_steps is and with or without a graph, every
    buffer unchanged: a required pointer NULL, n_rows != P, n_pool not the pool's rows, a range that is NaN, zero or negative (+inf passes),
    n_sets < 1, n_occ < 0, set_off or hp_off that decrease, start above 0 or end beyond the table, a nonzero reserved word, a run without
    retirement and scene; the stage call refuses the same way and a missing obs_skip too.  The scene's own refusals are inherited: the
    agent-sharded layout, a descriptor without obs_skip, step_staged() (the per-stage entry points carry no scene, so the stage cannot
    be staged from the host).  The tables' check is remembered per struct and made again for a struct that was set anew.  In Python:
    occlude() without a scene, a bad set_of, a bad range."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _blind(ctx, stock)
    before = sim.snapshot()
    good = sim._sight
    fields = {n: getattr(good, n) for n, _ in _lib.SightC._fields_}
    make = lambda **kw: _lib.SightC(**dict(fields, **kw))

    def refused(match, sight, desc=None):
        for graph in (False, True):
            for n in (0, 1):
                sim._sight, sim._desc = sight, desc
                with pytest.raises(MpcxError, match=match):
                    sim.run(n, graph)
        sim._sight, sim._desc = good, None
    for name in ('sight', 'n_seen', 'n_hidden', 'hp_off', 'set_off', 'set_of'):
        refused(r'mpcx error -1: sight: %s is null' % name, make(**{name: None}))
    refused(r'mpcx error -1: sight: hp or box is null', make(hp=None))
    refused(r'mpcx error -1: sight: hp or box is null', make(box=None))
    refused(r'mpcx error -1: sight: n_rows = 7 is not P = 8', make(n_rows=7))
    refused(r'mpcx error -1: sight: n_pool = 9 is not the run\'s 8 pool rows', make(n_pool=9))
    for bad in (float('nan'), 0.0, -1.0):
        refused(r'mpcx error -1: sight: range = .* must be positive', make(range=bad))
    refused(r'mpcx error -1: sight: n_sets = 0', make(n_sets=0))
    refused(r'mpcx error -1: sight: n_occ = -1 is negative', make(n_occ=-1))
    refused(r'mpcx error -1: sight: the reserved word is not 0', make(reserved=1))
    i32 = lambda v: ctx.i32(np.asarray(v, np.int32))
    for tab, match in (([0, 4, 3], 'set_off decreases at 1'), ([1, 4, 4], r'set_off\[0\] = 1 is not 0'), ([0, 4, 5], 'set_off ends at 5, beyond 4')):
        t = i32(tab)
        refused(r'mpcx error -1: sight: ' + match, make(set_off=t.data_ptr()))
    t = i32([0, 4, 8, 7, 16])
    refused(r'mpcx error -1: sight: hp_off decreases at 2', make(hp_off=t.data_ptr()))
    sim._sight = make(range=float('inf'))
    sim.run(0)
    sim._sight = good
    shard = sim._descriptor()
    shard.exchange, shard.n_inst, shard.agents_local, shard.obs_local = _lib.SHARD_AGENTS, 2, 4, sim.obs6.data_ptr()
    # inherited from the scene the stage lives on, which check_stages comes to first (the stage's own check has no branch for either)
    refused(r'mpcx error -1: scene: not supported in the agent-sharded layout', good, desc=shard)
    blind = sim._descriptor()
    blind.obs_skip = None
    refused(r'mpcx error -1: scene: obs_skip is required', good, desc=blind)
    # the offset tables are read back once per struct: a table broken in place under a struct that passed is checked again once the
    # struct has been taken off the context and set again
    tab = sim._sight_tabs[3]
    keep = tab.clone()
    sim.run(0)
    tab.copy_(i32([0, 4, 3]))
    ctx.set_sight(None)
    refused(r'mpcx error -1: sight: set_off decreases at 1', good)
    tab.copy_(keep)
    ctx.set_sight(None)
    sim.run(0)
    with pytest.raises(MpcxError, match='step_staged'):
        sim.step_staged()
    # the stage call: the same checks, and obs_skip
    args = (sim.state, sim.obs6, sim.obs_off, sim.obs_cnt)
    for bad, match in ((make(n_rows=3), 'sight: n_rows = 3'), (make(range=0.0), 'sight: range'), (make(set_of=None), 'set_of is null')):
        with pytest.raises(MpcxError, match=match):
            ctx.sight_step(*args, sim.obs_skip, bad, done=sim.done, absent=sim.absent)
    with pytest.raises(MpcxError, match='sight: no obs_skip'):
        ctx.sight_step(*args, None, good, done=sim.done, absent=sim.absent)
    ctx.synchronize()
    _same(sim.snapshot(), before, 'after the refusals')
    # a run without retirement and scene
    bare = _blind(ctx, stock)
    keep = bare._sight
    bare.keep_driving()
    assert bare._sight is None
    bare._sight = keep
    for n in (0, 1):
        with pytest.raises(MpcxError, match=r'mpcx error -1: sight: the run has no retirement and scene'):
            bare.run(n)
    bare._sight = None
    with pytest.raises(MpcxError, match='occlude: line of sight needs a scene'):
        bare.occlude([])
    for kw in (dict(set_of=np.array([0, 2])), dict(set_of=np.array([0])), dict(sensor_range=0.0), dict(sensor_range=float('nan')), dict(shrink=-1.0),
               dict(hear='everybody')):
        with pytest.raises(ValueError, match='occlude'):
            sim.occlude([[], []], **kw)
