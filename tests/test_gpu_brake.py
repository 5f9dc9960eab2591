"""Firm hold (mpcx_braking) on the device: the two stage calls against the host build of the rule byte for byte, the closed loop against
brake_helpers.BrakeOracleLoop step by step -- the queue scenes, the four-arm crossing, keep clear and the priority road on top, advice and
following beside it --, graph replay, host staging, off means off, the hold words following the stages of the run, and the refusals.
B = 2 instances, T = 13 everywhere.  The rule without a GPU is tests/test_brake_cpu.py.
Worst |GPU - oracle| over states and solutions seen on an MI355X (bar 2e-7): never green 4.6e-14, green 1.6e-13, four arms 1.3e-13, keep clear
on top 9.9e-14, priority road on top 1.5e-13, beside advice and following 1.9e-13."""
import numpy as np
import pytest
import torch

from tests import advise_helpers as AH
from tests import brake_helpers as BH
from tests import follow_helpers as FH
from tests import signal_helpers as G
from tests import test_gpu_follow as GF
from tests import test_gpu_respawn as GR
from tests import test_gpu_signal as TS

pytestmark = pytest.mark.gpu
TOL = 2e-7                      # the project's bar for states and solutions against the oracle
QUEUE_ROUTE = GF.QUEUE_ROUTE
NEVER = dict(cycle=100, amber=0, green=np.zeros((4, 2), dtype=np.int64))
AT_20 = dict(cycle=100, amber=0, green=np.tile(np.array([[20, 30]]), (4, 1)))        # the issue's green-at-60 plan with the clocks 40 steps on
BACK = (100, 145)


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
    return BH.build_ref(tmp_path_factory.mktemp('brake_ref'))


def _queue_tables(stock):
    from mpc_for_av_at_intersection_amd.batch import stop_lines
    routes = stock[0]
    stop, group = stop_lines(routes)
    o = int(sum(len(r) for r in routes[:QUEUE_ROUTE]))
    L = len(routes[QUEUE_ROUTE])
    stop[o:o + L] = np.where(np.arange(L) <= FH.QUEUE_LINE, FH.QUEUE_LINE, -1)
    group[o:o + L] = 0
    return stop, group


def _queue(c, stock, plan=NEVER, mode='speed', firm=True, retire=True):
    """B = 2 instances of one car on the straight route from the south, 100 and 145 points before the line of follow_helpers.queue_scene"""
    sim = GR._batch(c, stock, np.full((2, 1), QUEUE_ROUTE), np.array([[FH.QUEUE_LINE - b] for b in BACK]), mode)
    if not retire:
        sim.keep_driving()
    stop, group = _queue_tables(stock)
    sim.signalise(plan, stop=stop, group=group)
    if firm:
        sim.hold_firmly()
    return sim


def _snap(sim):
    out = sim.snapshot()
    if sim._signals is not None and sim._actuation is None and sim._reservation is None:
        out['tick'] = sim.tick.cpu().numpy().copy()
    return out


def _same(a, b, what, skip=()):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in b:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---------------------------------------------------------------- GB1: the stage calls against the host build
def _device_stage(c, w):
    """both stage calls on the words w (a dict of brake_helpers.words()); returns the words the device leaves"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    P, _, W = w['xref'].shape
    if c.params is None or c.params.T != W - 1:
        c.set_mpc_params(MpcParams(T=W - 1))
    i32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.int32, device=c.device)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=c.device)
    d = {k: i32(w[k]) for k in BH.I32_KEYS + BH.OPT_KEYS + ('path_stop', 'firm', 'win_len')}
    d.update({k: f64(w[k]) for k in BH.F64_KEYS + ('brake_cap',)})
    br = _lib.BrakingC(float(w['brake']), float(w['setback']), d['firm'].data_ptr(), d['overran'].data_ptr(), d['brake_cap'].data_ptr())
    c.brake_mark_step(float(w['dl']), _lib.STOP_SPEED if w['speed'] else _lib.STOP_CUT, d['path_off'], d['path_len'], d['traj_idx'], d['target_ind'],
                      d['win_len'], d['path_stop'], br, held=d['held'], boxed=d['boxed'], yielding=d['yielding'], done=d['done'])
    if w['speed']:
        c.brake_clamp_step(float(w['dl']), d['state'], d['path'], d['path_off'], d['path_len'], d['traj_idx'], d['path_stop'], br, d['xref'],
                           prev_len=d['len_seen'], done=d['done'])
    c.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


def _same_as_host(c, ref, w, what):
    host = BH.copy_words(w)
    n = BH.both_host(ref, host)
    got = _device_stage(c, w)
    for k, v in got.items():        # every word, written or not, byte for byte (the device's double sqrt and division are correctly rounded)
        if v is not None:
            assert v.tobytes() == host[k].tobytes(), (what, k, np.flatnonzero(v.ravel() != host[k].ravel())[:8])
    return n


@pytest.mark.parametrize('speed', [0, 1])
def test_stage_calls_on_hand_made_words(ctx, ref, speed):
    """GB1a.  mpcx_brake_mark_step_batch and mpcx_brake_clamp_step_batch on the hand-made words of tests/test_brake_cpu.py, with every hold
    word and with held switched off: every word equals the host build's, byte for byte, and nothing else is written"""
    w, want = BH.hand_made(speed)
    assert _same_as_host(ctx, ref, w, 'all') == 10
    w['held'] = None
    assert _same_as_host(ctx, ref, w, 'boxed and yielding') == 3


@pytest.mark.parametrize('W', [2, 14, 33])
@pytest.mark.parametrize('P', [1, 63, 65])
def test_stage_calls_on_random_words(ctx, ref, P, W):
    """GB1b.  Seeded random words of P agents with windows of W points -- one agent, one short of a wavefront of the mark and one beyond it;
    the clamp's sixteen agents a wavefront, 32, 4 or 1 of them a pass --, three seeds each, both stop modes, with and without the optional
    words: the same bytes as the host build"""
    held = 0
    for seed in range(3):
        held += _same_as_host(ctx, ref, BH.random_words(5000 + 64 * P + 8 * W + seed, P=P, W=W), (P, W, seed))
    assert held > 0 or P == 1


# ---------------------------------------------------------------- GB2: the closed loop against BrakeOracleLoop
def _sync(loop, before, rows):
    """the oracle loop's continuous words (and the indices the device carries) from the device's before the step; the rules' integers -- held,
    boxed, waited, yielding, the clocks, overran -- run on their own"""
    loop.state, loop.applied = before['state'][rows].copy(), before['applied'][rows].copy()
    loop.traj_idx, loop.target = [int(v) for v in before['traj_idx'][rows]], [int(v) for v in before['target_ind'][rows]]
    loop.prev = [int(v) for v in before['prev_cut'][rows]]
    loop.u = [before['u'][p].copy() for p in rows]


INT_WORDS = (('traj_idx', 'traj_idx'), ('cut', 'cut_len'), ('target', 'target_ind'), ('hit', 'hit_idx'), ('status', 'status'), ('held', 'held'),
             ('boxed', 'boxed'), ('yielding', 'yielding'), ('leader', 'leader'), ('firm', 'firm'), ('overran', 'overran'))


def _replay(sim, loops, n_steps):
    """n_steps of `sim`, every one replayed on the instances' oracle loops from the device's own state before the step.  After every step,
    for every driving agent: traj_idx (as the pin left it), cut_len, target index, hit, status, the hold words that are on, leader, firm and
    overran identical; brake_cap and row 2 of xref bit for bit; states and solutions within 2e-7.  Returns (worst difference, agent-steps
    held firmly, arrival steps)."""
    A = sim.A
    worst, n_firm = 0.0, 0
    arr = np.full(sim.P, -1)
    for s in range(n_steps):
        before = _snap(sim)
        sim.run(1)
        after = _snap(sim)
        for b, loop in enumerate(loops):
            rows = list(range(b * A, (b + 1) * A))
            assert [bool(d) for d in before['done'][rows]] == loop.done, (s, b)
            _sync(loop, before, rows)
            out = loop.step()
            for a, p in enumerate(rows):
                r = out[a]
                if r is None:
                    assert before['done'][p] and after['firm'][p] == 0 and after['brake_cap'][p] == 0.0, (s, p)
                    continue
                for mine, theirs in INT_WORDS:
                    if theirs in after:
                        want = r[mine] + b * A if mine == 'leader' and r[mine] >= 0 else r[mine]       # (a leader is a pool row)
                        assert int(after[theirs][p]) == want, (s, p, mine, after[theirs][p], want)
                assert after['brake_cap'][p].tobytes() == np.float64(r['brake_cap']).tobytes(), (s, p, after['brake_cap'][p], r['brake_cap'])
                if sim.stop_mode == 'speed':
                    assert np.array_equal(r['xref'][2], after['xref'][p, 2]), (s, p, r['xref'][2], after['xref'][p, 2])
                worst = max(worst, float(np.abs(r['u_sol'] - after['u'][p]).max()), float(np.abs(r['x_sol'] - after['x'][p]).max()),
                            float(np.abs(r['post'] - after['state'][p]).max()))
                assert bool(after['done'][p]) == loop.done[a], (s, p)
                n_firm += r['firm'] != 0
        arr[(arr < 0) & (after['done'] != 0)] = s + 1
        if after['done'].all():
            break
    assert worst < TOL, worst
    return worst, n_firm, arr


def _queue_loops(plan, tick=0, **kw):
    pl = dict(plan, green=np.asarray(plan['green'])[:1])
    return [BH.queue_loop(b, plan=pl, tick=[tick], **kw) for b in BACK]


def test_queue_in_front_of_a_light_that_never_turns_green(ctx, stock):
    """GB2a.  The never-green scene of tests/test_brake_cpu.py B5 as two instances (100 and 145 points back), 70 steps, against the oracle
    loop.  On the device too the cars stand behind their lines: traj_idx = 474 = s - 26, overran 0, |v| small.  THE SAME RUN WITH THE STAGE
    OFF has traj_idx on or past the line -- the assertion that fails without the feature."""
    sim = _queue(ctx, stock)
    worst, n_firm, arr = _replay(sim, _queue_loops(NEVER), 70)
    got = _snap(sim)
    print('never green: worst |GPU - oracle| %.2e, %d agent-steps held firmly, |v| %s' % (worst, n_firm, np.abs(got['state'][:, 2])))
    assert n_firm > 100 and (arr < 0).all() and got['traj_idx'].tolist() == [FH.QUEUE_LINE - 26] * 2 and got['overran'].tolist() == [0, 0]
    assert (got['firm'] == FH.QUEUE_LINE - 25).all() and sim.n_firm == 2 and (np.abs(got['state'][:, 2]) < 0.05).all()
    soft = _queue(ctx, stock, firm=False)
    soft.run(70)
    assert (_snap(soft)['traj_idx'] >= FH.QUEUE_LINE).all()


def test_queue_with_a_green(ctx, stock):
    """GB2b.  The green-at-60 scene with the clocks 40 steps on (green in steps 20 .. 49), 60 steps: held firmly until the green, then
    released; both cars arrive; every step equals the oracle loop's"""
    sim = _queue(ctx, stock, plan=AT_20)
    loops = _queue_loops(AT_20)
    worst, n_firm, arr = _replay(sim, loops, 60)
    print('green at 20: worst |GPU - oracle| %.2e, %d agent-steps held firmly, arrivals %s, passed %s' % (worst, n_firm, arr, [l.passed for l in loops]))
    assert n_firm > 10 and (arr > 20).all() and all(l.passed[0] >= 20 and l.over_line == [] for l in loops)


def test_four_arms_two_phases(ctx, stock):
    """GB2c.  The straight four-arm scene under two_phase_plan(100, 30, 8) as two instances, the second with its clocks 35 steps on, 70
    steps: every step equals the oracle loop's, and the two phases never mix"""
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    sim = TS._straight(ctx, stock, 'speed', offset=np.array([0, 35]))
    sim.hold_firmly()
    loops = [BH.straight_loop(tick=[t] * 4) for t in (0, 35)]
    worst, n_firm, arr = _replay(sim, loops, 70)
    print('four arms: worst |GPU - oracle| %.2e, %d agent-steps held firmly, arrivals %s' % (worst, n_firm, arr))
    assert n_firm > 100 and all(l.mixed_steps == [] and l.over_line == [] for l in loops)
    assert two_phase_plan(**G.PLAN)['cycle'] == 100


def test_keep_clear_on_top(ctx, stock):
    """GB2d.  The late-straight scene of keepclear_helpers in speed mode under its plan with keep clear, two instances (clocks 47 and 45),
    until everybody has arrived: boxed and held agents are held firmly, every step equals the oracle loop's"""
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    from tests import keepclear_helpers as KH
    ticks = (KH.LATE_TICK[True], KH.LATE_TICK[True] - 2)
    sim = GR._batch(ctx, stock, np.tile(np.array([[1, 3]]), (2, 1)), np.tile(np.array([KH.LATE_START[True]]), (2, 1)), 'speed')
    sim.signalise(two_phase_plan(**KH.LATE_PLAN), offset=np.array(ticks))
    sim.keep_clear()
    sim.hold_firmly()
    paths, dl, _, stop, group, move, ex, conflict = KH.late_tables()
    kc = dict(move=move, exit=ex, conflict=conflict, detect=max(int(s[0]) for s in stop))
    loops = [BH.BrakeOracleLoop(paths, dl, list(KH.LATE_START[True]), stop, group, two_phase_plan(**KH.LATE_PLAN), keepclear=kc, tick=[t] * 2, T=13,
                                depart=True, speed=True) for t in ticks]
    worst, n_firm, arr = _replay(sim, loops, 120)
    boxed = sum(int(l.boxed.sum()) for l in loops)
    print('keep clear on top: worst |GPU - oracle| %.2e, %d agent-steps held firmly, arrivals %s' % (worst, n_firm, arr))
    assert n_firm > 0 and (arr > 0).all() and boxed == 0 and all(l.over_line == [] for l in loops)


def test_priority_road_on_top(ctx, stock):
    """GB2e.  The two-car scene of priority_helpers in speed mode with the priority road and no signals, two instances (the minor car 60 and
    50 points into its route), until everybody has arrived: the yielding car is held firmly at the priority road's own stop line, every
    step equals the oracle loop's"""
    from tests import priority_helpers as PH
    starts = [PH.SCENES['two'][1], (0, 50)]
    sim = GR._batch(ctx, stock, np.tile(np.array(PH.SCENE_ROUTES['two']), (2, 1)), np.array(starts), 'speed')
    sim.priority_road(gap=PH.GAP_S, v_floor=PH.V_FLOOR_S)
    sim.hold_firmly()
    paths, dl, _, stop, group, move, ex, conflict, rank = PH.scene_tables('two')
    pr = dict(move=move, exit=ex, conflict=conflict, rank=rank, gap=PH.GAP_S, detect=max(int(s[0]) for s in stop), v_floor=PH.V_FLOOR_S)
    loops = [BH.BrakeOracleLoop(paths, dl, list(st), stop, group, priority=pr, T=13, depart=True, speed=True) for st in starts]
    worst, n_firm, arr = _replay(sim, loops, 150)
    print('priority road on top: worst |GPU - oracle| %.2e, %d agent-steps held firmly, arrivals %s' % (worst, n_firm, arr))
    assert n_firm > 0 and (arr > 0).all() and all(l.over_line == [] for l in loops)


def test_beside_advice_and_following(ctx, stock):
    """GB2f.  The queue of tests/test_gpu_follow.py (2 x 4 cars under signal_helpers.PLAN, red for another 40 and 25 steps) in speed mode
    with advise_speed(), follow() and the firm hold, 50 steps: all three clamps apply, every step equals the oracle loop's"""
    sim = GF._queue(ctx, stock, 'speed', advise=True)
    sim.hold_firmly()
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    paths, dl, _, stop, group = FH.queue_scene(4)
    follow = dict(FH.FOLLOW, **GF.WIDE)
    loops = [BH.BrakeOracleLoop(paths, dl, [int(v) for v in GF.QUEUE_START[b]], stop, group, two_phase_plan(**G.PLAN), follow=follow, advice=AH.ADVICE,
                                tick=[int(GF.OFFSET[b])] * 4, T=13, depart=True, speed=True) for b in range(2)]
    worst, n_firm, arr = _replay(sim, loops, 50)
    led = sum(l.followed_steps for l in loops)
    print('beside advice and following: worst |GPU - oracle| %.2e, %d agent-steps held firmly, %d with a leader' % (worst, n_firm, led))
    assert n_firm > 50 and led > 100


# ---------------------------------------------------------------- GB3: graph replay, host staging, off
def test_graph_replay_in_chunks(ctx, stock):
    """GB3.  The green-at-20 queue as 8 chunks of run(7, graph=True) on a side stream equals 56 x run(1) plain, byte for byte, firm, overran
    and brake_cap included"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    plain = _queue(ctx, stock, plan=AT_20)
    seen = 0
    for _ in range(56):
        plain.run(1)
        seen += plain.n_firm
    a = _snap(plain)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _queue(side, stock, plan=AT_20)
        torch.cuda.synchronize()
        for _ in range(8):
            graph.run(7, graph=True)
        _same(a, _snap(graph), 'graph')
        assert 'firm' in a and seen > 10
    finally:
        side.close()


def test_host_staging_equals_the_device_loop(ctx, stock):
    """GB4.  step_staged() with the firm hold equals run(1), every word, step by step over 30 steps of the never-green queue"""
    X, Y = (_queue(ctx, stock, retire=False) for _ in range(2))
    for s in range(30):
        X.run(1); Y.step_staged()
        _same(_snap(X), _snap(Y), s)
    assert X.n_firm == 2


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_off_means_off(ctx, stock, mode):
    """GB5.  hold_softly(), mpcx_set_braking(NULL) and an all-zero struct each give the bytes of a batch that never had the stage, and so
    does the stage ON with no agent held (a plan that is always green): 40 steps of the queue.  In cut mode the stage on differs from the
    stage off in its own words only."""
    from mpc_for_av_at_intersection_amd import _lib
    base = _queue(ctx, stock, mode=mode, firm=False); base.run(40)
    want = _snap(base)
    sim = _queue(ctx, stock, mode=mode); sim.hold_softly(); sim.run(40)
    _same(_snap(sim), want, 'hold_softly')
    assert (sim.firm == 0).all()            # never written
    sim = _queue(ctx, stock, mode=mode, firm=False)
    sim._claim_context(); sim.ctx.set_braking(_lib.BrakingC())
    sim._desc = sim._descriptor()
    sim.ctx.closed_loop_run(sim.ip, sim._desc, 40, False, **sim._stage_structs())
    _same(_snap(sim), want, 'zero struct')
    on = _queue(ctx, stock, mode=mode); on.run(40)
    got = _snap(on)
    own = ('firm', 'overran', 'brake_cap')
    if mode == 'cut':
        _same({k: v for k, v in got.items() if k not in own}, want, 'cut mode')
        assert (got['firm'] != 0).all() and (got['brake_cap'] == 0.0).all()
    else:
        assert got['state'].tobytes() != want['state'].tobytes() and (got['firm'] != 0).all()
    green = dict(cycle=100, amber=0, green=np.tile(np.array([[0, 100]]), (4, 1)))
    a, b = _queue(ctx, stock, plan=green, mode=mode), _queue(ctx, stock, plan=green, mode=mode, firm=False)
    a.run(40); b.run(40)
    got = _snap(a)
    _same({k: v for k, v in got.items() if k not in own}, _snap(b), 'nobody held')
    assert (got['firm'] == 0).all() and (got['brake_cap'] == 0.0).all() and (got['overran'] == 0).all()


def test_switching_the_holds_afterwards_is_honoured(ctx, stock):
    """GB6.  hold_firmly() first, then signals off and on and keep clear on: the hold words the stage reads are those of the stages that are
    on when the run is enqueued.  With the signals off (and no other source of stop lines) the run is refused in the stage's name; with them
    back on, and keep clear on top, the stage holds again and equals a batch that never lost its signals; with the priority road in their
    place the stale `held` words are not read."""
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    stop, group = _queue_tables(stock)
    sim = _queue(ctx, stock)
    sim.run(5)
    assert sim.n_firm == 2
    sim.unsignalise()
    assert sim._braking is not None
    with pytest.raises(MpcxError, match='braking: .*no source of stop lines'):
        sim.run(1)
    sim.signalise(NEVER, stop=stop, group=group, offset=np.array([5, 5]))
    sim.keep_clear()
    twin = _queue(ctx, stock)
    twin.run(5)
    twin.keep_clear()
    for s in range(20):
        sim.run(1); twin.run(1)
    a, b = _snap(sim), _snap(twin)
    for k in ('state', 'traj_idx', 'target_ind', 'firm', 'brake_cap', 'held', 'boxed', 'u', 'xref'):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert sim.n_firm == 2
    # signals off, the priority road on: the stale `held` words (red) are no longer read, and nobody yields in a junction of one car
    other = _queue(ctx, stock)
    other.run(5)
    other.unsignalise(); other.priority_road()
    other.run(3)
    assert other.n_firm == 0 and (other.held != 0).all() and (other.yielding == 0).all()


# ---------------------------------------------------------------- GB7: the refusals
def test_refusals(ctx, stock):
    """GB7.  MPCX_E_INVALID with a "braking: ..." message before anything is launched: a null word, brake or setback out of range, no source
    of stop lines, more than one linearisation pass, the agent-sharded layout; hold_firmly() refuses bad parameters itself"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _queue(ctx, stock)
    before = _snap(sim)
    good = sim._braking

    def run_with(struct, n=1, desc=None):
        sim._claim_context(); sim.ctx.set_braking(struct)
        if sim._desc is None:
            sim._desc = sim._descriptor()
        try:
            sim.ctx.closed_loop_run(sim.ip, sim._desc if desc is None else desc, n, False, **sim._stage_structs())
        finally:
            sim.ctx.set_braking(None)

    def variant(**kw):
        v = {n: getattr(good, n) for n, _ in _lib.BrakingC._fields_}
        v.update(kw)
        return _lib.BrakingC(*[v[n] for n, _ in _lib.BrakingC._fields_])

    cases = [(variant(firm=None), 'firm is null'), (variant(overran=None), 'overran is null'), (variant(brake_cap=None), 'brake_cap is null'),
             (variant(brake=0.0), 'brake'), (variant(brake=float('inf')), 'brake'), (variant(brake=-1.0), 'brake'),
             (variant(setback=1.9 * sim.dl), 'setback'), (variant(setback=float('nan')), 'setback')]
    for struct, msg in cases:
        for n in (0, 1):
            with pytest.raises(MpcxError, match='braking: .*' + msg):
                run_with(struct, n)
    free = _queue(ctx, stock, retire=False)         # (retirement refuses a second linearisation pass itself, in its own name)
    free._claim_context(); free._desc = free._descriptor()
    free.ctx.set_linearisation_passes(2)
    try:
        with pytest.raises(MpcxError, match='braking: .*linearisation pass'):
            free.ctx.closed_loop_run(free.ip, free._desc, 1, False, **free._stage_structs())
    finally:
        free.ctx.set_linearisation_passes(1); free.ctx.set_braking(None)
    shard = free._descriptor(); shard.exchange = _lib.SHARD_AGENTS        # (and a scene refuses the agent-sharded layout in its own name)
    free._claim_context()
    try:
        with pytest.raises(MpcxError, match='braking: .*agent-sharded'):
            free.ctx.closed_loop_run(free.ip, shard, 1, False, **free._stage_structs())
    finally:
        free.ctx.set_braking(None)
    _same(_snap(sim), before, 'nothing ran')
    for kw in (dict(brake=0.0), dict(brake=float('nan')), dict(setback=sim.dl)):
        with pytest.raises(ValueError, match='hold_firmly'):
            sim.hold_firmly(**kw)
    run_with(good, 1)       # and the good struct runs
    assert sim.n_firm == 2
