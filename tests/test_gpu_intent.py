"""GPU tests of SHARED PLANS in the device-resident closed loop (mpcx_closed_loop_run_intent, mpcx_interaction_batch_intent,
IntersectionBatch.share_plans): one launch between the prediction and the conflict search overwrites the predicted frames of a sharing
agent's own pool row with its last MPC solution re-rolled through the prediction's model.  The defining properties: a constant plan and
T = 1 leave the prediction stage's own frames BIT FOR BIT; a seeded plan equals the host build of the rule (csrc/mpcx_intent_core.h) within
the bound of the prediction test; every row that is not a sharing, driving, present agent's own keeps every bit; and every driving agent of
every closed-loop step equals the oracle step in which the others are seen on their plans (intent_helpers.intent_agent_step), which is
the step of intent_helpers.IntentOracleLoop.  Then: run(n), n x run(1), step_staged() and graph replay agree, off means off, the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import intent_helpers as IH
from tests import signal_helpers as G
from tests import test_gpu_scene as GS
from tests import test_gpu_signal as TS

pytestmark = pytest.mark.gpu

SHARE = np.array([1, 0, 1, 1, 1, 1, 0, 1])         # a mixed fleet: B = 2 instances of four agents
OFFSET = np.array([60, 75])                        # the signal clocks of the two instances (tests/test_gpu_advise.py's)
STEPS = 30


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
    return IH.build_ref(tmp_path_factory.mktemp('intent_ref'))


# ---------------------------------------------------------------- the stage call
class Stage:
    """P agents on one stock path in a pool of P + 3 rows (the three rows in the middle are nobody's own: scripted cars; obs_skip is
    the agents' own rows, as ego_row is with traffic), windows of at most eight rows, seeded poses and controls."""

    def __init__(self, ctx, P, seed):
        self.ctx, self.P = ctx, P
        rng = np.random.default_rng(seed)
        full = H.gold('mpc_pre.npz')['path_4_1']
        self.n_path = len(full)
        self.d_full = ctx.f64(full)
        self.d_cs = ctx.f64(np.column_stack([np.cos(full[:, 2]), np.sin(full[:, 2])]))
        self.n_pool = P + 3
        self.own = (np.arange(P) + 3 * (np.arange(P) >= P // 2)).astype(np.int32)
        self.idx = rng.integers(0, len(full) - 200, P).astype(np.int32)
        self.state = np.column_stack([full[self.idx, 0], full[self.idx, 1], rng.uniform(0, 9, P), full[self.idx, 2]])
        n = self.n_pool
        self.pool = np.column_stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(0, 9, n), rng.uniform(-np.pi, np.pi, n),
                                     rng.uniform(-2, 2, n), rng.uniform(-0.4, 0.4, n)])
        self.pool[self.own, :4] = self.state
        self.off = np.clip(self.own - 4, 0, max(n - 8, 0)).astype(np.int32)
        self.cnt = np.full(P, min(8, n), np.int32)
        self.car = H.car()

    def ip(self, S):
        from mpc_for_av_at_intersection_amd.runtime import InteractionParams
        car = self.car
        return InteractionParams(pred_steps=int(S), frame_window=20, cutoff_margin=4, L=car['L'], radius=car['radius'],
                                 circle_centers=np.array(car['circle_centers']).ravel())

    def run(self, S, u=None, share=None, status=None, done=None, absent=None, intent=None, own=None, pool=True):
        """one mpcx_interaction_batch (u is None) or mpcx_interaction_batch_intent -> (prediction (n_pool, S, 4), frames or None)"""
        from mpc_for_av_at_intersection_amd import _lib
        c, P = self.ctx, self.P
        kw, frames = {}, None
        if u is not None or intent is not None:
            d_share = c.i32(np.ones(P) if share is None else share)
            frames = c.i32(np.full(P, -7))
            self.keep = (d_share, frames)
            kw = dict(intent=_lib.IntentC(d_share.data_ptr(), frames.data_ptr(), P, 0) if intent is None else intent,
                      u_sol=c.f64(u), status=c.i32(np.zeros(P) if status is None else status),
                      done=None if done is None else c.i32(done), absent=None if absent is None else c.i32(absent))
        c.interaction(self.ip(S), c.f64(self.state), self.d_full, self.d_cs, c.i32(np.zeros(P)), c.i32(np.full(P, self.n_path)),
                      c.i32(self.idx + 1), c.f64(self.pool) if pool else None, c.i32(self.off), c.i32(self.cnt),
                      c.i32(self.own if own is None else own), c.i32(self.idx), **kw)
        pred = c.interaction_prediction(self.n_pool, S).reshape(self.n_pool, S, 4)
        return pred, None if frames is None else frames.cpu().numpy()

    def words(self, S, u, base, **kw):
        cc = np.array(self.car['circle_centers']).ravel()
        return IH.words(state=self.state, u_sol=u, status=kw.get('status', np.zeros(self.P)), obs_skip=self.own,
                        share=kw.get('share', np.ones(self.P)), done=kw.get('done'), absent=kw.get('absent'), pred=base.copy(), dt=0.2,
                        L=self.car['L'], cc=cc)


def _set_T(ctx, T, car):
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    ctx.set_mpc_params(MpcParams(T=int(T), L=car['L']))


SHAPES = [(T, S) for T in (1, 2, 5, 20) for S in (1, 4, 35, IH.PRED_STEPS_MAX)]


@pytest.mark.parametrize('P', [1, 3, 64, 65])
def test_constant_plan_and_horizon_one_bitwise(ctx, P):
    """S1.  P in {1, 3, 64, 65} (one group, less than a wavefront's sixteen agents, four full wavefronts = one block, one agent into the
    next block) x T in {1, 2, 5, 20} x pred_steps in {1, 4, 35, 64}.  A plan whose columns j >= 1 hold the pool row's controls (column 0
    is seeded noise; with T = 1 column 0 IS the applied control) leaves every bit of the same call without the stage, frames = pred_steps
    everywhere.  Not vacuous: a seeded plan with T >= 2 does change every agent's row."""
    st = Stage(ctx, P, 10 + P)
    rng = np.random.default_rng(P)
    for T, S in SHAPES:
        _set_T(ctx, T, st.car)
        base, none = st.run(S)
        assert none is None
        u = np.repeat(st.pool[st.own][:, 4:6, None], T, axis=2)
        if T > 1:
            u[:, :, 0] = rng.uniform(-1, 1, (P, 2))
        got, frames = st.run(S, u=u)
        assert got.tobytes() == base.tobytes(), (T, S, np.argwhere(got != base)[:4])
        assert (frames == S).all(), (T, S, frames)
        if T > 1:
            other, _ = st.run(S, u=u + 0.05)
            assert all((other[r] != base[r]).any() for r in st.own), (T, S)
            rest = np.setdiff1d(np.arange(st.n_pool), st.own)
            assert other[rest].tobytes() == base[rest].tobytes(), (T, S)


@pytest.mark.parametrize('P', [1, 3, 64, 65])
def test_seeded_plans_against_the_host_build(ctx, ref, P):
    """S2.  The same shapes with seeded plans and, per agent, about one time in five each: share = 0, done, its own row absent, a failed
    status (any of MAXITER, INFEASIBLE, NUMERIC).  The rows taken from plans equal the host build of the rule within 1e-13 -- the bound
    tests/test_oracle_golden.py puts on the oracle's prediction: the same chain length, the device's sincos and tan against the C
    library's --; frames equals the host build's; every other row -- non-sharing, done, absent, failed, and the three rows that are
    nobody's own -- keeps every bit of the call without the stage.  Once with done and absent not given.
    The bound is absolute and was set on poses within 62 m of the origin (the recorded predictions' extent: starts within 30 m, 7 s at up to
    9 m/s in every direction), where one unit in the last place is at most 7e-15.  So that it means here what it means there, the poses
    stay in that range: starts on the path (within 30 m), and speeds and accelerations drawn so that the displacement over the
    t = pred_steps x dt seconds of a case is at most 16 + 8 m: v0 in [0, min(9, 16 / t)], acc in +-min(2, 16 / t^2)."""
    st = Stage(ctx, P, 20 + P)
    rng = np.random.default_rng(100 + P)
    worst, taken = 0.0, 0
    v_unit = rng.uniform(0, 1, P)
    for T, S in SHAPES:
        _set_T(ctx, T, st.car)
        t = 0.2 * S
        st.state[:, 2] = v_unit * min(9.0, 16.0 / t)
        st.pool[st.own, :4] = st.state
        base, _ = st.run(S)
        a_max = min(2.0, 16.0 / (t * t))
        u = np.stack([rng.uniform(-a_max, a_max, (P, T)), rng.uniform(-0.4, 0.4, (P, T))], axis=1)
        rare = lambda n: (rng.random(n) < 0.2).astype(np.int32)
        for masks in (True, False):
            kw = dict(share=1 - rare(P), status=rare(P) * rng.integers(1, 4, P))
            if masks:
                kw.update(done=rare(P), absent=rare(st.n_pool))
            w = st.words(S, u, base, **kw)
            n = IH.host_rule(ref, w)
            got, frames = st.run(S, u=u, **kw)
            assert frames.tolist() == w['frames'].tolist(), (T, S)
            rows = st.own[w['frames'] > 0]
            rest = np.setdiff1d(np.arange(st.n_pool), rows)
            assert got[rest].tobytes() == base[rest].tobytes(), (T, S, masks)
            if len(rows):
                worst = max(worst, float(np.abs(got[rows] - w['pred'][rows]).max()))
            taken += n
    print('P = %d: %d rows taken from plans, worst |device - host build| = %.2e' % (P, taken, worst))
    assert taken > 0 and worst <= IH.PRED_TOL, worst


# ---------------------------------------------------------------- the closed loop
def _shared(c, stock, share=SHARE, retire=True, mode='speed'):
    """B = 2 instances of the four straight routes from index 0 under signals (tests/test_gpu_signal.py's scene), plans shared by `share`
    (None: never shared)"""
    sim = TS._straight(c, stock, mode, offset=OFFSET, retire=retire)
    if share is not None:
        sim.share_plans(share)
    return sim


def _oracle_params(sim):
    from oracle import oracle_py as orc
    return orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})


def _plans(sim, before, share):
    """per agent: (state, u) if the others see it on its plan in the step that starts from `before`, else None"""
    own = sim.obs_skip.cpu().numpy()
    out = []
    for q in range(sim.P):
        ok = share[q] and before['status'][q] == 0
        if 'done' in before:
            ok = ok and not before['done'][q] and not before['absent'][own[q]]
        out.append((before['state'][q], before['u'][q]) if ok else None)
    return out


def _replay_step(sim, before, after, pool, tabs, share):
    """Every DRIVING agent of the step replayed on the oracle with the others seen on their plans (intent_helpers.intent_agent_step, the
    step of IntentOracleLoop).  traj_idx, the stop index, hit_idx, target_ind, status and held identical, u and x within 2e-7 (the bar of
    tests/test_gpu_advise.py's loop); shared_frames is pred_steps exactly for the agents seen on their plans."""
    po = _oracle_params(sim)
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    cc = np.asarray(sim.ip.circle_centers, dtype=np.float64).ravel()
    S = int(sim.ip.pred_steps)
    speed = sim.stop_mode == 'speed'
    stop = sim.stop_index() if speed else None
    retire = 'done' in before
    absent = before['absent'] if retire else np.zeros(len(pool), np.int32)
    plans = _plans(sim, before, share)
    assert after['shared_frames'].tolist() == [S if p is not None else 0 for p in plans]
    row_agent = {int(o_skip[q]): q for q in range(sim.P)}
    seen = {}
    worst, n_hit = 0.0, 0
    for p in range(sim.P):
        plan = int(tabs['plan_of'][p])
        cycle = int(tabs['plan_cycle'][plan])
        t = int(before['tick'][p]) % cycle
        if retire and before['done'][p]:
            continue
        present = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p] and not absent[r]]
        for r in present:
            if r not in seen:
                seen[r] = IH.seen_trajectory(po, pool[r], plans[row_agent[r]] if r in row_agent else None, cc, S)

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
        r = IH.intent_agent_step(po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], [seen[k] for k in present], int(before['traj_idx'][p]),
                                 int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                                 sim.ip.cutoff_margin, speed, decide, v_ref=sim.v_ref if speed else None)
        want_hit = -1 if r['hit'] is None else int(r['hit'][2])
        want = (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status, r['held'])
        cut = stop[p] if speed else after['cut_len'][p]
        got = (after['traj_idx'][p], cut, after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p])
        assert want == tuple(int(v) for v in got), (p, want, got)
        worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
        n_hit += want_hit >= 0
    print('    step: worst |GPU - oracle| %.2e, %d agents in conflict' % (worst, n_hit))
    assert worst < 2e-7, worst
    return worst, n_hit


def test_closed_loop_on_the_oracle(ctx, stock):
    """L1.  Two instances of the four straight routes in speed mode under signal_helpers.PLAN (clocks 60 and 75), a mixed fleet (agents 1
    and 6 do not share), 30 steps.  After every step every driving agent equals (a) the oracle step from the device's own state of the
    step before with the others seen on their plans, and (b) the step of the free-running IntentOracleLoop of its instance: integer
    decisions identical, u and x within 2e-7.  shared_frames is pred_steps for the sharing agents."""
    sim = _shared(ctx, stock)
    tabs = TS._tables(sim)
    paths, dl, start, stop, group = G.straight_scene()
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    cpu = [IH.IntentOracleLoop(paths, dl, start, stop, group, two_phase_plan(**G.PLAN), share=SHARE[4 * b:4 * b + 4], tick=[int(OFFSET[b])] * 4,
                               T=13, depart=True, speed=True) for b in range(2)]
    worst, drift, hits = 0.0, 0.0, 0
    stop_idx = None
    for s in range(STEPS):
        before = TS._snap(sim)
        sim.run(1)
        after = TS._snap(sim)
        w, h = _replay_step(sim, before, after, GS._pool_before(sim, before, after), tabs, SHARE)
        worst, hits = max(worst, w), hits + h
        stop_idx = sim.stop_index()
        for b in range(2):
            out = cpu[b].step()
            for a in range(4):
                p = 4 * b + a
                if out[a] is None:
                    assert before['done'][p]
                    continue
                o = out[a]
                want = (o['traj_idx'], o['cut'], o['target'], o['hit'], o['status'], o['held'])
                got = (after['traj_idx'][p], stop_idx[p], after['target_ind'][p], after['hit_idx'][p], after['status'][p], after['held'][p])
                assert want == tuple(int(v) for v in got), (s, p, want, got)
                drift = max(drift, float(np.abs(o['u_sol'] - after['u'][p]).max()), float(np.abs(o['x_sol'] - after['x'][p]).max()))
    print('closed loop: worst |GPU - oracle step| %.2e, worst |GPU - IntentOracleLoop| %.2e over %d steps, %d agent-steps in conflict'
          % (worst, drift, STEPS, hits))
    assert drift < 2e-7, drift


def test_run_chunks_staging_and_graph_agree(ctx, stock):
    """L2.  run(30) = 30 x run(1) = 30 x step_staged() (mpcx_interaction_batch_intent in the place of mpcx_interaction_batch) = 30 replays
    of the captured step on a side stream, byte for byte on every snapshot() key, shared_frames included; the mixed fleet, no retirement
    (step_staged() has no retired mask)."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    whole, single, staged = (_shared(ctx, stock, retire=False) for _ in range(3))
    whole.run(STEPS)
    for _ in range(STEPS):
        single.run(1)
        staged.step_staged()
    a = TS._snap(whole)
    TS._same(TS._snap(single), a, 'n x run(1)', skip=())
    TS._same(TS._snap(staged), a, 'step_staged', skip=())
    assert a['shared_frames'].tolist() == (SHARE * int(whole.ip.pred_steps)).tolist()
    side = Context(0, stream=torch.cuda.Stream(device=0))
    try:
        graph = _shared(side, stock, retire=False)
        torch.cuda.synchronize()
        for _ in range(3):
            graph.run(STEPS // 3, graph=True)
        TS._same(TS._snap(graph), a, 'graph', skip=())
    finally:
        side.close()


def test_off_means_off(ctx, stock):
    """L3.  share all-zero, intent = NULL and an all-zero struct through mpcx_closed_loop_run_intent, and keep_plans_private(), each give
    the bytes of a batch that never shared on every snapshot() key they have in common, 30 steps; with share all-zero shared_frames is
    zero.  The batch that does share is seen differently: its prediction of the last step differs from the twin's in the sharing agents'
    rows and in no other."""
    from mpc_for_av_at_intersection_amd import _lib
    base = _shared(ctx, stock, share=None)
    base.run(STEPS)
    want = TS._snap(base)
    S = int(base.ip.pred_steps)
    pred_base = ctx.interaction_prediction(base.P, S)
    runs = {}
    sim = _shared(ctx, stock, share=np.zeros(8, np.int32)); sim.run(STEPS); runs['share all-zero'] = sim
    sim = _shared(ctx, stock, share=None); _entry(sim, None, STEPS); runs['NULL'] = sim
    sim = _shared(ctx, stock, share=None); _entry(sim, _lib.IntentC(), STEPS); runs['zero struct'] = sim
    sim = _shared(ctx, stock); sim.keep_plans_private(); sim.run(STEPS); runs['keep_plans_private'] = sim
    for name, sim in runs.items():
        got = TS._snap(sim)
        frames = got.pop('shared_frames', None)
        assert (frames is not None) == (name == 'share all-zero') and (frames is None or not frames.any()), name
        TS._same(got, want, name, skip=())
    assert not runs['keep_plans_private'].shared_frames.any()           # no longer written
    # one more step from the same state, seen on plans: only the sharing agents' rows differ
    twin = runs['NULL']
    twin.share_plans(SHARE)
    base.run(1)
    pred_free = ctx.interaction_prediction(base.P, S)
    twin.run(1)
    pred_shared = ctx.interaction_prediction(base.P, S)
    differs = [bool((pred_shared[r] != pred_free[r]).any()) for r in range(base.P)]
    live = (want['done'] == 0) & (want['status'] == 0)
    print('rows that differ when seen on plans: %s (sharing %s, driving %s)' % (differs, SHARE.tolist(), live.astype(int).tolist()))
    assert not any(d and not t for d, t in zip(differs, ((SHARE != 0) & live).tolist())) and sum(differs) >= 4
    assert twin.shared_frames.cpu().numpy().tolist() == (((SHARE != 0) & live) * S).tolist()
    assert pred_base.shape == pred_free.shape


def _twins(make, warm, share):
    """two batches from make() run `warm` steps without sharing (identical), then one shares: -> (free, shared)"""
    a, b = make(), make()
    a.run(warm); b.run(warm)
    b.share_plans(share)
    return a, b


def _rows_after_one_step(c, sim, rows):
    before = sim.snapshot()
    sim.run(1)
    return before, c.interaction_prediction(rows, int(sim.ip.pred_steps)).reshape(rows, int(sim.ip.pred_steps), 4), sim.snapshot()


def _host_rows(sim, ref, before, pred, share, done=None, absent=None):
    cc = np.asarray(sim.ip.circle_centers, dtype=np.float64).ravel()
    w = IH.words(state=before['state'], u_sol=before['u'], status=before['status'], obs_skip=sim.obs_skip.cpu().numpy(), share=share, done=done,
                 absent=absent, pred=pred.copy(), dt=float(sim.ip.dt), L=float(sim.ip.L), cc=cc)
    IH.host_rule(ref, w)
    return w


def test_masks_in_the_loop(ctx, stock, ref):
    """L4.  Ten steps without sharing on two identical batches, then everybody shares on one; agent 2 is marked done, the row of agent 5
    absent (with done, as a departed car is) and the status of agent 7 failed, on both.  After one more step the prediction of the sharing
    batch equals the twin's bit for bit in the rows of agents 2, 5 and 7, and the host build of the rule applied to the twin's prediction
    within 1e-13 elsewhere; shared_frames is 0 for the three."""
    a, b = _twins(lambda: _shared(ctx, stock, share=None), 10, np.ones(8, np.int32))
    for sim in (a, b):
        sim.done[2] = 1; sim.done[5] = 1; sim.absent[5] = 1; sim.sol['status'][7] = 1
    ctx.synchronize()
    S = int(a.ip.pred_steps)
    _, free, _ = _rows_after_one_step(ctx, a, a.P)
    before, got, after = _rows_after_one_step(ctx, b, b.P)
    w = _host_rows(b, ref, before, free, np.ones(8), done=before['done'], absent=before['absent'])
    assert after['shared_frames'].tolist() == w['frames'].tolist() == [S, S, 0, S, S, 0, S, 0]
    for r in (2, 5, 7):
        assert got[r].tobytes() == free[r].tobytes(), r
    rows = [0, 1, 3, 4, 6]
    worst = float(np.abs(got[rows] - w['pred'][rows]).max())
    print('masks: worst |device - host build| %.2e' % worst)
    assert worst <= IH.PRED_TOL and all((got[r] != free[r]).any() for r in rows)


def test_scripted_traffic_rows_are_untouched(ctx, stock, ref):
    """L5.  One instance of two agents and the stock pair of scripted cars (obs_skip = ego_row; cut mode), ten steps, then both agents
    share: after one more step the scripted cars' rows equal the twin's bit for bit, the agents' rows the host build within 1e-13."""
    a, b = _twins(lambda: GS._pair(ctx, stock, backs=(20.0,), traffic=True), 10, None)
    rows = int(a.obs6.shape[0])
    _, free, _ = _rows_after_one_step(ctx, a, rows)
    before, got, after = _rows_after_one_step(ctx, b, rows)
    ego = b.ego_row.cpu().numpy().tolist()
    assert b.obs_skip.cpu().numpy().tolist() == ego and rows >= 4 and len(set(range(rows)) - set(ego)) >= 2
    w = _host_rows(b, ref, before, free, np.ones(2), done=before['done'], absent=before['absent'])
    for r in range(rows):
        if r in ego:
            assert np.abs(got[r] - w['pred'][r]).max() <= IH.PRED_TOL and (got[r] != free[r]).any(), r
        else:
            assert got[r].tobytes() == free[r].tobytes(), r
    assert after['shared_frames'].tolist() == [int(b.ip.pred_steps)] * 2


def test_right_of_way_keeps_its_standing_records(ctx, stock, ref):
    """L6.  The straight scene with give_way(fixed words), ten steps, then the mixed fleet shares: after one more step the standing
    records equal the twin's bit for bit, the non-sharing agents' frames too, the sharing agents' frames the host build within 1e-13, and
    shared_frames is as specified."""
    def make():
        sim = _shared(ctx, stock, share=None)
        sim.give_way(order=np.tile(np.arange(4), (2, 1)))
        return sim
    a, b = _twins(make, 10, SHARE)
    S = int(a.ip.pred_steps)
    _, free, _ = _rows_after_one_step(ctx, a, a.P)
    stand_free = a.stand.cpu().numpy().copy()
    before, got, after = _rows_after_one_step(ctx, b, b.P)
    assert b.stand.cpu().numpy().tobytes() == stand_free.tobytes() and stand_free.any()
    w = _host_rows(b, ref, before, free, SHARE, done=before['done'], absent=before['absent'])
    assert after['shared_frames'].tolist() == w['frames'].tolist() == (SHARE * S).tolist()
    for r in range(b.P):
        if SHARE[r]:
            assert np.abs(got[r] - w['pred'][r]).max() <= IH.PRED_TOL and (got[r] != free[r]).any(), r
        else:
            assert got[r].tobytes() == free[r].tobytes(), r


# ---------------------------------------------------------------- the refusals
def _entry(sim, intent, n, graph=0, desc=None):
    """mpcx_closed_loop_run_intent itself, with the structs of `sim`"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip = sim.ip.to_c()
    byref = lambda s: None if s is None else C.byref(s)
    c = sim.ctx
    c._chk(c.lib.mpcx_closed_loop_run_intent(c._ctx, C.byref(cip), C.byref(sim._desc if desc is None else desc), None, byref(sim._opts),
                                             byref(sim._retire), byref(sim._scene), byref(sim._admit), byref(sim._respawn), byref(sim._routes),
                                             byref(sim._precedence), byref(sim._signals), byref(sim._actuation), byref(sim._advice),
                                             byref(intent), int(n), int(graph)))
    if desc is None:
        sim.steps_done += n


def test_refusals(ctx, stock):
    """L7.  MPCX_E_INVALID with an "intent: ..." message before anything is launched, whatever n_steps is and with or without a graph,
    every buffer unchanged: share NULL, frames NULL, n_rows != P, an obs_skip outside the pool, the agent-sharded exchange, no pool --
    through the loop entry; the stage call refuses the same (it has no exchange).  In Python: share_plans() with a malformed array or an
    agent-sharded exchange."""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = TS._straight(ctx, stock, 'speed', plans=None, retire=False)       # (no scene and no signals: their own checks of obs_skip and
    sim.share_plans(SHARE)                                                  # of the exchange would speak first)
    before = TS._snap(sim)
    sim._desc = sim._descriptor()
    it = sim._intent
    good = {n: getattr(it, n) for n, _ in _lib.IntentC._fields_}
    make = lambda **kw: _lib.IntentC(**dict(good, **kw))
    copy = lambda **kw: _set(type(sim._desc).from_buffer_copy(sim._desc), **kw)

    def _set(d, **kw):
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(match, intent, desc=None):
        for graph in (0, 1):
            for n in (0, 1):
                with pytest.raises(MpcxError, match=match):
                    _entry(sim, intent, n, graph, desc=desc if desc is not None else copy())
    refused(r'mpcx error -1: intent: share is null', make(share=None))
    refused(r'mpcx error -1: intent: frames is null', make(frames=None))
    for n in (0, 7, 9, -8):
        refused(r'mpcx error -1: intent: n_rows = %d is not P = 8' % n, make(n_rows=n))
    for row, where in ((8, 3), (-1, 0), (1 << 20, 7)):
        bad = sim.obs_skip.clone(); bad[where] = row
        ctx.synchronize()
        refused(r'mpcx error -1: intent: agent %d has own pool row obs_skip = %d outside the pool of 8' % (where, row), it, copy(obs_skip=bad.data_ptr()))
    refused(r'mpcx error -1: intent: needs obs_skip', it, copy(obs_skip=None))
    refused(r'mpcx error -1: intent: not in the agent-sharded layout', it, copy(exchange=_lib.SHARD_AGENTS))
    refused(r'mpcx error -1: intent: no pool', it, copy(obs6=None))
    # ---- the stage call
    st = Stage(ctx, 5, 3)
    _set_T(ctx, 5, st.car)
    u = np.zeros((5, 2, 5))
    base, _ = st.run(4)
    d_share, frames = ctx.i32(np.ones(5)), ctx.i32(np.zeros(5))
    ok = dict(share=d_share.data_ptr(), frames=frames.data_ptr(), n_rows=5, reserved=0)
    bad_own = st.own.copy(); bad_own[4] = st.n_pool
    for match, kw in ((r'intent: share is null', dict(intent=_lib.IntentC(**dict(ok, share=None)))),
                      (r'intent: frames is null', dict(intent=_lib.IntentC(**dict(ok, frames=None)))),
                      (r'intent: n_rows = 4 is not P = 5', dict(intent=_lib.IntentC(**dict(ok, n_rows=4)))),
                      (r'intent: share is null', dict(intent=_lib.IntentC())),
                      (r'intent: agent 4 has own pool row obs_skip = 8 outside the pool of 8', dict(own=bad_own)),
                      (r'intent: no pool', dict(pool=False))):
        with pytest.raises(MpcxError, match=match):
            st.run(4, u=u, **kw)
    assert ctx.interaction_prediction(st.n_pool, 4).tobytes() == base.tobytes() and not frames.cpu().numpy().any()
    ctx.synchronize()
    TS._same(TS._snap(sim), before, 'refused', skip=())
    assert sim.steps_done == 0 and not sim.shared_frames.any()
    # ---- Python
    for bad in (np.ones(7, np.int32), np.ones((2, 4), np.int32), np.ones(8), ['a'] * 8):
        with pytest.raises(ValueError, match='share_plans'):
            sim.share_plans(bad)
    assert sim._intent is it
    sim.share_plans(SHARE != 0)                  # a bool array is accepted
    assert sim.share.cpu().numpy().tolist() == SHARE.tolist()
    keep = sim.exchange
    try:
        for ex in ('rccl', lambda rows: rows):
            sim.exchange = ex
            with pytest.raises(MpcxError, match='agent-sharded'):
                sim.share_plans()
            with pytest.raises(MpcxError, match='agent-sharded'):
                sim.run(1)
    finally:
        sim.exchange = keep
    sim.keep_plans_private()
    assert sim._intent is None and 'shared_frames' not in sim.snapshot()
