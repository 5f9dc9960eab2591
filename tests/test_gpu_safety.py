"""GPU tests of THE NEAR-MISS LOG in the device-resident closed loop (mpcx_set_safety, IntersectionBatch.watch_safety): one launch behind the
conflict search names every driving agent's nearest vehicle and its first predicted contact, keeps a table of encounters on the device, and
mpcx_safety_summary reduces it to a conflict matrix.  The stage entry equals the host build of the rule; inside the loop its clearance is
the run log's byte for byte and its contact words are the numpy rule on the prediction read back; a run with the stage on leaves every
other buffer as it was; off means off; graph replay; respawn; the refusals; the matrix.  B = 2, A = 4, T = 13, v0 = 0."""
import numpy as np
import pytest
import torch

from tests import safety_helpers as SF
from tests import test_gpu_follow as GF
from tests import test_gpu_respawn as GR
from tests import test_gpu_scene as GS
from tests import test_gpu_signal as TS
from tests.test_safety_cpu import _matrix_table

pytestmark = pytest.mark.gpu

STEPS = 40
SAFETY_KEYS = ('partner', 'near_clearance', 'ttc_row', 'ttc_frame', 'n_events')
# the device's sincos and hypot are a few ulp from libm's: the bar of the run-log tests
DEVICE_TOL = 1e-9


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
    return SF.build_ref(tmp_path_factory.mktemp('safety_ref'))


# ---------------------------------------------------------------- G1: the stage entry against the host build
def _device_stage(ctx, w):
    """mpcx_safety_step_batch on the words w (a dict of safety_helpers.words()) with its synthetic prediction; returns the words it leaves"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams
    P, n_pool, S, cap = len(w['traj_idx']), len(w['obs6']), w['pred'].shape[1], w['capacity']
    i32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.int32, device=ctx.device)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=ctx.device)
    d = {k: i32(w[k]) for k in SF.I32_KEYS + SF.OPT_KEYS + ('row_agent',) + SF.OUT_I32}
    d.update({k: f64(w[k]) for k in ('state', 'obs6', 'clearance', 'ev_f64')})
    d['pred'] = f64(w['pred']).reshape(n_pool, S, 2, 2)
    s = _lib.SafetyC(d['partner'].data_ptr(), d['clearance'].data_ptr(), d['ttc_row'].data_ptr(), d['ttc_frame'].data_ptr(), d['tick'].data_ptr(),
                     d['enc_row'].data_ptr(), d['n_events'].data_ptr(), d['ev_i32'].data_ptr() if cap else None,
                     d['ev_f64'].data_ptr() if cap else None, d['row_agent'].data_ptr(), w['near'], w['ttc_frames'], cap, P, n_pool, 0)
    ip = InteractionParams(pred_steps=S, radius=w['radius'], circle_centers=w['cc'])
    ctx.safety_step(ip, d['state'], d['path_off'], d['traj_idx'], d['obs6'], d['obs_off'], d['obs_cnt'], d['obs_skip'], s, pred=d['pred'],
                    done=d['done'], absent=d['absent'])
    ctx.synchronize()
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}
    got['pred'] = got['pred'].reshape(n_pool, S, 4)
    return got


def _same_as_host(ctx, ref, w, what):
    host = SF.copy_words(w)
    SF.host_rule(ref, host)
    got = _device_stage(ctx, w)
    try:
        SF.same_words(got, host, DEVICE_TOL)        # integer words, ttc_*, ticks and event integers exact; clearance and ev_f64 within 1e-9
    except AssertionError as e:
        raise AssertionError((what,) + e.args)
    for k in SF.I32_KEYS + SF.OPT_KEYS + ('row_agent', 'state', 'obs6', 'pred'):       # nothing else is written
        if w[k] is not None:
            assert got[k].tobytes() == w[k].tobytes(), (what, k)
    return host


@pytest.mark.parametrize('S,near,ttc_frames', [(35, 1.5, 5), (1, 1.5, 1), (35, 0.0, 0)])
def test_stage_entry_on_hand_made_words(ctx, ref, S, near, ttc_frames):
    """G1a.  mpcx_safety_step_batch on the hand-made words of tests/test_safety_cpu.py (N1) with their synthetic prediction: the host
    build's words -- which N1 checks against the values written down by hand --, and on the scripted sequence of N2 at capacity 8, 1 and
    0 the host build's events after every step"""
    w, _ = SF.hand_made(S=S, near=near, ttc_frames=ttc_frames)
    host = _same_as_host(ctx, ref, w, 'hand')
    assert (host['partner'] >= 0).sum() == 12
    for cap in (8, 1, 0):
        w, frames = SF.sequence_words(cap)
        for s, (obs6, pred) in enumerate(frames):
            w['obs6'], w['pred'] = np.ascontiguousarray(obs6), np.ascontiguousarray(pred)
            w = _same_as_host(ctx, ref, w, ('sequence', cap, s))
        assert w['n_events'].tolist() == [3, 0] and w['tick'].tolist() == [8, 8]


@pytest.mark.parametrize('P', [5, 17, 33])
def test_stage_entry_on_random_scenes(ctx, ref, P):
    """G1b.  Seeded random scenes of P = 5, 17 and 33 agents (a ragged last lane group, a ragged wavefront, a ragged block) with 0..19 others
    each and a synthetic prediction of 1, 2, 7 and 35 frames; six seeds per P.  The two smallest distances of every agent differ by more
    than 1e-6 (asserted on the host), so the partner cannot hinge on the few ulp between the device's sincos / hypot and libm's."""
    partners = contacts = 0
    for seed in range(6):
        w = SF.random_words(2000 + 16 * P + seed, P=P, S=(35, 1, 2, 7, 35, 35)[seed])
        assert SF.margin_numpy(w) > 1e-6, (P, seed)
        host = _same_as_host(ctx, ref, w, (P, seed))
        partners += int((host['partner'] >= 0).sum()); contacts += int((host['ttc_frame'] >= 0).sum())
    assert partners > 2 * P and contacts > 0


# ---------------------------------------------------------------- G2: inside the loop
def _traffic(ctx, stock, mode='cut'):
    """the stock scripted-traffic scene: the four straight routes from index 0 and the stock scenario's two scripted cars per instance"""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_specs
    cd = stock[2]
    return GR._batch(ctx, stock, TS.STRAIGHT, np.zeros((2, 4), dtype=np.int64), mode,
                     traffic=scripted_traffic_specs(2, 2, 0, cd.distance_back_to_front_wheel, dt=0.2))


# the four straight routes from staggered start indices some 13 - 19 m along: the cars reach the crossing within the 40 steps, one after the
# other (from index 0 they are still on their approach arms after 40 steps and no contact is ever predicted)
STAGGER = np.array([[220, 180, 200, 160], [230, 170, 210, 150]])


def _shared(ctx, stock, mode='cut', share=True, retire=True):
    """four cars on the four straight routes from STAGGER, every one sharing its plan"""
    sim = GR._batch(ctx, stock, TS.STRAIGHT, STAGGER, mode)
    if not retire:
        sim.keep_driving()
    if share:
        sim.share_plans()
    return sim


def _numpy_step(sim, before, after, pred):
    """the numpy rule's searches on the step before -> after: the pool the step saw, the prediction read back, traj_idx as the conflict
    search left it; per agent (r_now, c_now, r_ttc, k_ttc, the difference between its two smallest distances)"""
    rows = int(sim.obs6.shape[0])
    s = sim._safety
    w = SF.words(state=before['state'], traj_idx=after['traj_idx'], path_off=sim.path_off.cpu().numpy(), done=before.get('done'),
                 absent=before.get('absent'), row_agent=sim._row_agent.cpu().numpy(), obs6=GS._pool_before(sim, before, after),
                 pred=pred.reshape(rows, -1, 4), obs_off=sim.obs_off.cpu().numpy(), obs_cnt=sim.obs_cnt.cpu().numpy(),
                 obs_skip=sim.obs_skip.cpu().numpy(), radius=sim.ip.radius, cc=np.asarray(sim.ip.circle_centers).ravel(), near=s.near,
                 ttc_frames=s.ttc_frames, capacity=0)
    out = []
    for q in range(sim.P):
        d = []
        found = SF.search_numpy(w, q, d)
        d = sorted(d)
        out.append(found + (d[1] - d[0] if len(d) > 1 else np.inf,))
    return out


@pytest.mark.parametrize('scene', ['traffic', 'shared'])
def test_inside_the_loop(ctx, stock, scene):
    """G2.  40 steps of run(1) of the stock scripted-traffic scene (2 x [4 agents | 2 scripted cars]) and of a four-car scene with shared
    plans on, the run log attached.  After every step ttc_frame and ttc_row equal the numpy rule applied to mpcx_interaction_prediction's
    read-back, the partner is the numpy rule's (wherever the two nearest differ by more than 1e-6) and the clearance within 1e-9 of it; and for every driving agent the clearance equals the
    run log's clearance column of the same step byte for byte.  Not vacuous: contacts are predicted, and nobody is ever without a
    partner."""
    sim = _traffic(ctx, stock) if scene == 'traffic' else _shared(ctx, stock)
    log = sim.attach_log(STEPS)
    sim.watch_safety(near=0.5, ttc=2.0)
    rows, S = int(sim.obs6.shape[0]), int(sim.ip.pred_steps)
    seen, n_ttc, n_partner = [], 0, 0
    for s in range(STEPS):
        before = TS._snap(sim)
        sim.run(1)
        after = TS._snap(sim)
        want = _numpy_step(sim, before, after, ctx.interaction_prediction(rows, S))
        for q, (r_now, c_now, r_ttc, k_ttc, margin) in enumerate(want):
            assert (after['ttc_row'][q], after['ttc_frame'][q]) == (r_ttc, k_ttc), (s, q, want[q])
            assert after['partner'][q] == r_now or margin <= 1e-6, (s, q)        # (the straight routes are mirror images: two cars can be equally near)
            assert (after['partner'][q] >= 0) == (r_now >= 0), (s, q)
            assert (c_now == after['near_clearance'][q]) if np.isinf(c_now) else abs(c_now - after['near_clearance'][q]) <= DEVICE_TOL, (s, q)
        n_ttc += int((after['ttc_frame'] >= 0).sum()); n_partner += int((after['partner'] >= 0).sum())
        seen.append((before['done'].copy(), after['near_clearance'].copy()))
    logged = log.rows()['clearance']
    compared = 0
    for s, (done, clr) in enumerate(seen):
        drive = done == 0
        assert logged[s][drive].tobytes() == clr[drive].tobytes(), (s, logged[s], clr)
        assert np.isinf(clr[~drive]).all()
        compared += int(drive.sum())
    ev = sim.near_misses()
    print('%s: %d agent-steps with a predicted contact, %d with a partner, %d compared with the log, %d events' % (scene, n_ttc, n_partner, compared, len(ev)))
    assert n_ttc > 0 and compared > 200 and n_partner >= compared and len(ev) > 0
    assert sim._safety_tick.cpu().numpy().tolist() == [STEPS] * sim.P
    # the matrix of these events against numpy (the classes: every stock route)
    offs = sim._route_offs[:-1].astype(np.int32)
    ni, nf = SF.summary_numpy(sim.A, offs, sim.ip.dt, sim.n_events.cpu().numpy(), sim._ev_i32.cpu().numpy(), sim._ev_f64.cpu().numpy())
    cm = sim.conflict_matrix()
    assert cm.shape == (2, len(offs) + 1, len(offs) + 1) and cm['events'].sum() == len(ev)
    assert np.array_equal(np.stack([cm['events'], cm['contacts'], cm['predicted']], -1), ni)
    assert np.stack([cm['min_clearance'], cm['min_ttc']], -1).tobytes() == nf.tobytes()
    if scene == 'traffic':
        assert cm['events'][:, :, -1].sum() == (ev['partner_path_off'] < 0).sum() == (ev['row'] % 6 >= 4).sum()      # the scripted cars' rows


# ---------------------------------------------------------------- G3: behaviour unchanged
def _without(snap):
    return {k: v for k, v in snap.items() if k not in SAFETY_KEYS}


@pytest.mark.parametrize('mode', ['cut', 'speed'])
def test_behaviour_unchanged(ctx, stock, mode):
    """G3.  The queue of tests/test_gpu_follow.py under signals and following (and advice in speed mode), the run log attached, 40 steps:
    the batch with the stage on leaves every other buffer of snapshot() and every row and outcome word of the run log byte-identical to
    the batch without it -- and the stage did see something"""
    sims, logs = [], []
    for watch in (False, True):
        sim = GF._queue(ctx, stock, mode, advise=mode == 'speed')
        logs.append(sim.attach_log(STEPS))
        if watch:
            sim.watch_safety(near=8.0, ttc=3.0)
        sim.run(STEPS)
        sims.append(sim)
    a, b = (TS._snap(s) for s in sims)
    assert all(k in b for k in SAFETY_KEYS) and not any(k in a for k in SAFETY_KEYS)
    TS._same(_without(b), a, 'stage on', skip=())
    assert logs[0].rows().tobytes() == logs[1].rows().tobytes()
    oa, ob = logs[0].outcomes(), logs[1].outcomes()
    assert all(oa[k].tobytes() == ob[k].tobytes() for k in oa)
    assert b['n_events'].sum() > 0 and (b['partner'] >= 0).any()


# ---------------------------------------------------------------- G4: off
def _run_raw(sim, safety, n, graph=0, desc=None):
    """the widest entry point with the structs of `sim` and `safety` set on the context by hand"""
    sim._claim_context()
    sim.ctx.set_safety(safety)
    if sim._desc is None:
        sim._desc = sim._descriptor()
    try:
        sim.ctx.closed_loop_run(sim.ip, sim._desc if desc is None else desc, n, bool(graph), **sim._stage_structs())
    finally:
        sim.ctx.set_safety(None)


def test_off_means_off(ctx, stock):
    """G4.  mpcx_set_safety(NULL), an all-zero struct, and watch_safety() followed by stop_watching() each give the bytes of a batch that
    never had the stage, and write none of its words.  Host staging (step_staged) with the stage on equals run(1), its words included."""
    from mpc_for_av_at_intersection_amd import _lib
    base = _shared(ctx, stock)
    base.run(STEPS)
    want = TS._snap(base)
    runs = {}
    sim = _shared(ctx, stock); _run_raw(sim, None, STEPS); runs['NULL'] = sim
    sim = _shared(ctx, stock); _run_raw(sim, _lib.SafetyC(), STEPS); runs['zero struct'] = sim
    sim = _shared(ctx, stock); sim.watch_safety(); sim.run(3); sim.stop_watching(); sim.run(STEPS - 3); runs['stop_watching'] = sim
    for name, sim in runs.items():
        got = TS._snap(sim)
        assert 'partner' not in got
        TS._same(got, want, name, skip=())
    assert runs['stop_watching']._safety_tick.cpu().numpy().tolist() == [3] * 8         # not written after the stage was cleared
    X, Y = (_shared(ctx, stock, share=False, retire=False) for _ in range(2))
    for sim in (X, Y):
        sim.watch_safety(near=3.0, ttc=4.0)
    for s in range(10):
        X.run(1); Y.step_staged()
        TS._same(TS._snap(X), TS._snap(Y), s, skip=())
    assert X.near_misses().tobytes() == Y.near_misses().tobytes() and len(X.near_misses()) > 0


# ---------------------------------------------------------------- G5: graph replay
def test_graph_replay():
    """G5.  The four-car scene with shared plans: 8 chunks of run(5, graph=True) on a side stream equal 40 x run(1) plain byte for byte, the
    stage's words and events included; the tick keeps advancing over the replays (40 after eight of them); and the cached graph's key
    covers the struct by value: `near` changed in place between two replayed runs equals the same sequence run plain -- and differs from
    the run that kept it."""
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        stock = stock_routes(side)
        sims = []
        for _ in range(3):
            sim = _shared(side, stock)
            sim.watch_safety(near=0.5, ttc=1.0)
            sims.append(sim)
        torch.cuda.synchronize()
        for sim, graph, change in zip(sims, (True, False, True), (True, True, False)):
            sim.run(5, graph=graph); sim.run(5, graph=graph)
            assert sim._safety_tick.cpu().numpy().tolist() == [10] * 8
            if change:
                sim._safety.near = 25.0
            for _ in range(6):
                sim.run(5, graph=graph)
        a, b, c = (TS._snap(sim) for sim in sims)
        TS._same(a, b, 'replay against plain', skip=())
        TS._same(_without(a), _without(c), 'the stage decides nothing', skip=())
        assert sims[0].near_misses().tobytes() == sims[1].near_misses().tobytes()
        assert all(sim._safety_tick.cpu().numpy().tolist() == [STEPS] * 8 for sim in sims)
        assert a['n_events'].sum() > c['n_events'].sum()
    finally:
        side.close()


# ---------------------------------------------------------------- G6: respawn
def test_words_survive_a_slot_reset(ctx, stock):
    """G6.  Four cars near the end of one route, each slot serving two vehicles (respawn, the second due at step 60, gap 0), near = 50 m so that
    every measured step is critical: 80 steps.  n_events never falls, the tick is the step count for every slot whether it drives, waits or has
    been reset, and the table of a slot that has been reset holds events of both its vehicles: one opened before the first vehicle's
    arrival and one opened after the second entered; the reset itself closed what was open."""
    sim = GF._queue(ctx, stock, 'cut', signals=False, follow=None, start=np.array([[600, 500, 400, 300], [610, 505, 400, 295]]))
    due = np.zeros((2, 4, 2), dtype=np.int64); due[..., 1] = 60
    sim.respawn_on_schedule(due, gap=0.0)
    sim.watch_safety(near=50.0, ttc=0.0, capacity=16)
    last = np.zeros(8, np.int64)
    for s in range(80):
        sim.run(1)
        n = sim.n_events.cpu().numpy()
        assert (n >= last).all() and sim._safety_tick.cpu().numpy().tolist() == [s + 1] * 8
        last = n
    ep, ev = sim.episodes(), sim.near_misses()
    print(ep, ev[['agent', 'open', 'last', 'row']])
    reset = [int(q) for q in np.unique(ep['slot'])]
    assert reset, 'no slot was reset'
    both = 0
    for q in reset:
        first = ep[(ep['slot'] == q) & (ep['generation'] == 0)][0]
        mine = ev[ev['agent'] == q]
        assert (mine['open'] <= first['arrived']).any(), q
        both += bool((mine['open'] >= 60).any())
        assert not ((mine['open'] <= first['arrived']) & (mine['last'] > first['arrived'])).any(), q       # the reset closed the encounter
    assert both > 0
    assert (ev['path_off'] == int(sim.path_off.cpu().numpy()[0])).all()


# ---------------------------------------------------------------- G7: the refusals
def test_refusals(ctx, stock):
    """G7.  MPCX_E_INVALID with a "safety: ..." message before anything is launched, whatever n_steps is and with or without a graph, every
    buffer unchanged: each required pointer NULL; an event array NULL with capacity > 0; n_rows != P; n_pool not the run's pool rows;
    near negative or not finite; ttc_frames outside 0..pred_steps; a negative capacity; a nonzero reserved word; the agent-sharded
    layout.  The stage call refuses the same way.  In Python: watch_safety() with malformed values."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = TS._straight(ctx, stock, 'cut', plans=None, retire=False)
    sim.watch_safety()
    before = TS._snap(sim)
    s0 = sim._safety
    names = [n for n, _ in _lib.SafetyC._fields_]
    good = {n: getattr(s0, n) for n in names}
    make = lambda **kw: _lib.SafetyC(**dict(good, **kw))

    def refused(match, safety, staged=True, **kw):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _run_raw(sim, safety, n, graph, **kw)
        if staged:
            with pytest.raises(MpcxError, match=match):
                ctx.safety_step(sim.ip, sim.state, sim.path_off, sim.traj_idx, sim.obs6, sim.obs_off, sim.obs_cnt, sim.obs_skip, safety)
    for name in ('partner', 'clearance', 'ttc_row', 'ttc_frame', 'tick', 'enc_row', 'n_events', 'row_agent'):
        refused(r'mpcx error -1: safety: %s is null' % name, make(**{name: None}))
    for name in ('ev_i32', 'ev_f64'):
        refused(r'mpcx error -1: safety: ev_i32 or ev_f64 is null with capacity = 8', make(**{name: None}))
    for n in (0, 7, 9, -8):
        refused(r'mpcx error -1: safety: n_rows = %d is not P = 8' % n, make(n_rows=n))
    for n in (0, 7, 9, -8):
        refused(r'mpcx error -1: safety: n_pool = %d is not the run\'s 8 pool rows' % n, make(n_pool=n))
    for v in (-0.5, float('inf'), float('nan')):
        refused(r'mpcx error -1: safety: near = .* must be finite and not negative', make(near=v))
    for v in (-1, 36):
        refused(r'mpcx error -1: safety: ttc_frames = %d outside 0\.\.pred_steps = 35' % v, make(ttc_frames=v))
    refused(r'mpcx error -1: safety: capacity = -1 is negative', make(capacity=-1))
    refused(r'mpcx error -1: safety: the reserved word is not 0', make(reserved=1))
    _run_raw(sim, make(near=0.0, ttc_frames=0, capacity=0, ev_i32=None, ev_f64=None), 0)        # the limits themselves are accepted
    _run_raw(sim, make(ttc_frames=35), 0)
    desc = sim._descriptor()
    desc.exchange = _lib.SHARD_AGENTS
    refused('mpcx error -1: safety: not supported in the agent-sharded layout', s0, staged=False, desc=desc)
    desc = sim._descriptor()
    desc.obs_skip = None
    refused('mpcx error -1: safety: the descriptor has no obs_skip', s0, staged=False, desc=desc)
    ctx.synchronize()
    TS._same(TS._snap(sim), before, 'refused', skip=())
    assert sim.steps_done == 0 and (sim.partner == -1).all() and not sim.n_events.any() and not sim._safety_tick.any()
    for kw in (dict(near=-1.0), dict(near=float('nan')), dict(ttc=-1.0), dict(ttc=float('inf')), dict(capacity=-1)):
        with pytest.raises(ValueError):
            sim.watch_safety(**kw)
    assert sim._safety is s0
    sim.stop_watching()
    assert sim._safety is None and 'partner' not in sim.snapshot()


# ---------------------------------------------------------------- G8: the conflict matrix
def test_conflict_matrix_on_a_hand_made_table(ctx, ref):
    """G8.  mpcx_safety_summary on the hand-made event table of tests/test_safety_cpu.py (N4: an actor partner, an unknown offset, a NaN
    clearance, a record beyond n_events, more events than are stored, two routes with one offset): the host build's tables byte for
    byte, with three routes and with none; and on a table of 3 x 70 agents with up to 5 stored events each (more than one pass of the
    wavefront over an instance), seeded, against numpy"""
    n_events, ev_i32, ev_f64, routes = _matrix_table()
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device=ctx.device)
    for ro in (routes, np.zeros(0, np.int32)):
        hi, hf = SF.host_summary(ref, 2, ro, 0.2, n_events, ev_i32, ev_f64)
        gi, gf = ctx.safety_summary(2, dev(ro, torch.int32), 0.2, dev(n_events, torch.int32), dev(ev_i32, torch.int32), dev(ev_f64, torch.float64))
        ctx.synchronize()
        assert gi.cpu().numpy().tobytes() == hi.tobytes() and gf.cpu().numpy().tobytes() == hf.tobytes()
    rng = np.random.default_rng(5)
    P, A, cap = 210, 70, 5
    n_events = rng.integers(0, 9, P).astype(np.int32)
    ev_i32 = rng.integers(-1, 35, (P, cap, 8)).astype(np.int32)
    ev_i32[..., 4:6] = rng.choice([-1, 0, 700, 1400, 2100, 9999], (P, cap, 2))
    ev_f64 = rng.uniform(-1.0, 4.0, (P, cap, 2))
    ev_f64[rng.random((P, cap)) < 0.05, 0] = np.nan
    ro = np.array([0, 700, 1400, 2100], np.int32)
    ni, nf = SF.summary_numpy(A, ro, 0.2, n_events, ev_i32, ev_f64)
    gi, gf = ctx.safety_summary(A, dev(ro, torch.int32), 0.2, dev(n_events, torch.int32), dev(ev_i32, torch.int32), dev(ev_f64, torch.float64))
    ctx.synchronize()
    assert gi.cpu().numpy().tobytes() == ni.tobytes() and gf.cpu().numpy().tobytes() == nf.tobytes()
    assert ni[..., 0].sum() == np.minimum(n_events, cap).sum() and (ni[:, -1].sum() > 0) and (ni[:, :, -1].sum() > 0)
