"""GPU tests of the run log of the device-resident closed loop (record_kernel, csrc/mpcx_record.hip): the reference's recorded stock
scenario logged in ONE run(n) -- goal arrival = the reference's loop length, rows = its History --, the log against per-step
snapshots of a twin batch (bit-identical; same rows from the staged path and from graph replays, whose cursor must live on the device),
clearance and outcomes against numpy, the single-ego and agent-sharded layouts, capacity rules and the refusals.  The host build of the
same rule is tests/test_runlog_cpu.py."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_traffic import _stock_batch
from tests.test_runlog_cpu import GOAL_DIS, STOP_SPEED, numpy_clearance, outcome_from_clearances

pytestmark = pytest.mark.gpu

INTS = ('traj_idx', 'target_ind', 'cut_len', 'hit_idx', 'status', 'iters')


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


def _family(c, stock, B=24, A=3, K=2, T=13, seed=3):
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    routes, dl, cd = stock
    return scripted_traffic_batch(c, B=B, A=A, K=K, T=T, seed=seed, routes=routes, dl=dl, cd=cd)


def _assert_rows_equal(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for name in a.dtype.names:
        assert np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == 'f'), (what, name)


@pytest.mark.parametrize('T', [10, 13, 20])
def test_stock_run_in_one_call(ctx, T):
    """main/scenarios/mpc_intersection.py:95-159 -- the ego on path (4, 1) and the two scripted cars -- 8 copies, a log attached, ONE
    run(steps): goal_step = the reference's number of loop iterations for every copy, rows = the recorded run (state after each step and
    controls within 1e-6, the bar of test_recorded_stock_closed_loop_on_the_device; integer decisions exact, status 0), history() = the
    reference's History, and the car that spawns on the ego's start pose is no contact"""
    g = H.gold('closedloop.npz')
    pre = 'T%d/' % T
    n = int(g[pre + 'steps'])
    B = 8
    sim, full = _stock_batch(ctx, T, 'generated', B)
    log = sim.attach_log(n)
    sim.run(n)
    out = log.outcomes()
    rows = log.rows()
    assert rows.shape == (n, B)
    print('T=%d: goal_step %s, golden %d; min_clearance %.4f, clearance at step 0 %.6f' % (T, out['goal_step'].tolist(), n, out['min_clearance'][0],
                                                                                           rows['clearance'][0, 0]))
    assert (out['goal_step'] == n).all(), out['goal_step']
    assert (out['steps'] == n).all()
    st = np.stack([rows[k] for k in ('x', 'y', 'v', 'yaw')], axis=-1)                  # (n, B, 4)
    ds = float(np.abs(st[:-1] - g[pre + 'state'][1:, None, :]).max())
    du = float(np.abs(np.stack([rows['steer'], rows['accel']], axis=-1) - g[pre + 'ctrl'][:, None, :]).max())
    print('T=%d: worst |state - golden| %.2e, worst |control - golden| %.2e' % (T, ds, du))
    assert ds < 1e-6 and du < 1e-6
    hit = np.where(g[pre + 'hit'][:, 2] >= 0, g[pre + 'hit'][:, 2], -1).astype(np.int64)
    for name, want in (('traj_idx', g[pre + 'tidx']), ('target_ind', g[pre + 'target']), ('cut_len', g[pre + 'cut']), ('hit_idx', hit)):
        assert np.array_equal(rows[name], np.repeat(want[:, None], B, axis=1)), name
    assert (rows['status'] == 0).all() and (rows['iters'] >= 0).all() and rows['iters'].max() > 0       # (0 iterations: solved by the trial pass)
    # xref_deviation: the formula on the golden's own numbers.  It measures from the state before the step, which the device holds within the
    # 1e-6 bar above in x and in y: the two components move by at most 1e-6 each, their hypot by at most 1.5e-6
    pt = full[g[pre + 'target']]
    ang = pt[:, 2] + np.pi / 2
    dev = np.hypot(np.cos(ang) * (pt[:, 0] - g[pre + 'ox'][:, 0, 0]), np.sin(ang) * (pt[:, 1] - g[pre + 'ox'][:, 1, 0]))
    assert np.abs(rows['xref_deviation'] - dev[:, None]).max() < 1.5e-6 and dev.max() > 0.15
    # the second scripted car stands on the ego's start pose for its start delay: raw clearance -2 radius, and NOT a contact
    assert np.abs(rows['clearance'][0] + 2 * sim.ip.radius).max() < 1e-9
    assert (out['contact_step'] == -1).all() and (out['min_clearance'] > 1.0).all()
    # the last row comes from the plant step the recorded run ends with
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from mpc_for_av_at_intersection_amd.lib.simulation import Simulation, State
    x, y, v, yaw = g[pre + 'state'][-1]
    last = Simulation(BicycleModelDimensions(), 0.2, State(x=x, y=y, yaw=yaw, v=v)).step(g[pre + 'ctrl'][-1][1], g[pre + 'ctrl'][-1][0])
    assert np.abs(st[-1] - np.array([last.x, last.y, last.v, last.yaw])).max() < 1e-6
    # History of copy 3: the initial state first, then one entry per step, n + 1 in all, times from the class itself
    h = log.history(3)
    assert len(h.x) == n + 1 == len(h.t) and h.a[0] == 0.0 and h.delta[0] == 0.0 and h.xref_deviation[0] == 0.0
    assert np.abs(np.array([h.x[0], h.y[0], h.v[0], h.yaw[0]]) - g[pre + 'state'][0]).max() < 1e-6 and h.x[0] == log.initial[3, 0]
    assert np.array_equal(h.x[1:], rows['x'][:, 3]) and np.array_equal(h.a[1:], rows['accel'][:, 3]) and np.array_equal(h.delta[1:], rows['steer'][:, 3])
    assert np.allclose(np.diff(h.t), 0.2) and abs(h.t[0] - 0.2) < 1e-15
    # nothing is frozen at the goal: further steps are recorded (beyond the capacity they are dropped) and history() still ends at the goal
    sim.run(2)
    assert (log.outcomes()['steps'] == n + 2).all() and (log.outcomes()['goal_step'] == n).all() and log.rows().shape == (n, B)
    assert len(log.history(0).x) == n + 1


def _snap_rows(snaps, P):
    from mpc_for_av_at_intersection_amd.batch import RUN_LOG_DTYPE
    out = np.zeros((len(snaps), P), RUN_LOG_DTYPE)
    for s, sn in enumerate(snaps):
        for k, name in enumerate(('x', 'y', 'v', 'yaw')):
            out[name][s] = sn['state'][:, k]
        out['steer'][s], out['accel'][s] = sn['applied'][:, 0], sn['applied'][:, 1]
        for name in INTS:
            out[name][s] = sn[name]
    return out


def test_the_log_is_the_run(ctx, stock):
    """scripted_traffic_batch(B = 24, A = 3, K = 2, T = 13, seed = 3), 12 steps: the rows written by ONE run(12) are bit-identical to the
    snapshots collected with 12 x run(1) on a twin batch without a log (state, applied, the six integers), and the twin's final snapshot
    equals the logged batch's -- attaching a log changes no result.  The same rows come from step_staged() and from graph replays of
    5 + 7 steps on a side stream: the per-agent cursor lives on the device, so the second replay continues at row 5 (a cursor kept on the
    host would write rows 0..4 twice).  After detach_log() the batch runs on as its twin does."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    n = 12
    logged, twin, staged = _family(ctx, stock), _family(ctx, stock), _family(ctx, stock)
    P = logged.P
    log = logged.attach_log(n)
    logged.run(n)
    snaps = []
    for _ in range(n):
        twin.run(1)
        snaps.append(twin.snapshot())
    rows = log.rows()
    want = _snap_rows(snaps, P)
    for name in ('x', 'y', 'v', 'yaw', 'accel', 'steer') + INTS:
        assert np.array_equal(rows[name], want[name]), name
    final = logged.snapshot()
    for k, v in snaps[-1].items():
        assert np.array_equal(v, final[k]), k
    assert (rows['status'] == 0).all() and rows['v'].max() > 1.0 and np.isfinite(rows['clearance']).all() and np.isfinite(rows['xref_deviation']).all()
    assert (log.outcomes()['steps'] == n).all()
    # stage by stage through mpcx_record_step_batch
    slog = staged.attach_log(n)
    for _ in range(n):
        staged.step_staged()
    _assert_rows_equal(slog.rows(), rows, 'staged')
    # graph replays on a side stream
    side = Context(0, stream=torch.cuda.Stream(device=0))
    gr = _family(side, stock)
    glog = gr.attach_log(n)
    torch.cuda.synchronize()
    gr.run(5, graph=True)
    gr.run(7, graph=True)
    assert (glog.outcomes()['steps'] == n).all()
    _assert_rows_equal(glog.rows(), rows, 'graph')
    for name, other in (('staged', slog), ('graph', glog)):
        a, b = log.outcomes(), other.outcomes()
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k)
    gsnap = gr.snapshot()
    for k, v in final.items():
        assert np.array_equal(v, gsnap[k]), ('graph', k)
    # detached: today's launches again, on the plain and on the graph path (the cached graph with the record stage must not be replayed)
    assert logged.detach_log() is log and gr.detach_log() is glog
    logged.run(3)
    gr.run(3, graph=True)
    twin.run(3)
    t = twin.snapshot()
    for name, s in (('plain', logged.snapshot()), ('graph', gr.snapshot())):
        for k, v in t.items():
            assert np.array_equal(v, s[k]), (name, k)
    assert (log.outcomes()['steps'] == n).all() and (glog.outcomes()['steps'] == n).all()
    side.close()


def test_clearance_and_outcomes_against_numpy(ctx, stock):
    """the same family, 60 steps.  Every step's clearance of every ego recomputed with numpy from the log's own poses of the other egos
    (row s - 1; the initial state for s = 0) and the scripted cars' poses from the host classes: within 1e-9 m (the device's actor poses
    are within 1e-11 of the classes', tests/test_gpu_traffic.py, its sincos within a few ulp).  goal_step, contact_step and
    min_clearance recomputed from the log's rows must equal the device's EXACTLY, for every agent: they are comparisons and minima of
    stored values."""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_specs
    from mpc_for_av_at_intersection_amd.lib import moving_obstacles as mo
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    routes, dl, cd = stock
    B, A, K, n = 24, 3, 2, 60
    sim = _family(ctx, stock)
    log = sim.attach_log(n)
    sim.run(n)
    sim.check()
    rows, out = log.rows(), log.outcomes()
    assert rows.shape == (n, B * A) and (out['steps'] == n).all()
    spec = scripted_traffic_specs(B, K, 3, cd.distance_back_to_front_wheel)
    bic = BicycleModelDimensions()
    with contextlib.redirect_stdout(io.StringIO()):
        tapes = np.stack([mo.MovingObstacleTIntersection(bic, direction=int(a['direction']), turning=bool(a['turning']), speed=float(a['speed']),
                                                         offset=float(a['offset']), dt=0.2).tape(n) for a in spec.actors], axis=1)    # (n, B * K, 6)
    post = np.stack([rows['x'], rows['y'], rows['yaw']], axis=-1)                            # (n, P, 3)
    start = np.concatenate([log.initial[None][:, :, [0, 1, 3]], post[:-1]]).reshape(n, B, A, 3)
    cars = tapes[:, :, [0, 1, 3]].reshape(n, B, K, 3)
    want = np.zeros((n, B, A))
    for s in range(n):
        for b in range(B):
            for a in range(A):
                others = np.concatenate([np.delete(start[s, b], a, axis=0), cars[s, b]])
                want[s, b, a] = numpy_clearance(start[s, b, a], others, cd)
    got = rows['clearance'].reshape(n, B, A)
    worst = float(np.abs(got - want).max())
    print('clearance vs numpy: worst %.3e m over %d agent-steps; range %.3f .. %.3f m' % (worst, got.size, got.min(), got.max()))
    assert worst <= 1e-9
    # outcomes from the rows
    path = sim.path.cpu().numpy()
    off, ln = sim.path_off.cpu().numpy().astype(np.int64), sim.path_len.cpu().numpy().astype(np.int64)
    goal = path[off + ln - 1]
    there = ((np.hypot(rows['x'] - goal[:, 0], rows['y'] - goal[:, 1]) <= GOAL_DIS) & (np.abs(rows['target_ind'] - rows['cut_len']) < 5) &
             (np.abs(rows['v']) <= STOP_SPEED))
    want_goal = np.where(there.any(axis=0), there.argmax(axis=0) + 1, -1)
    assert np.array_equal(out['goal_step'], want_goal)
    outc = [outcome_from_clearances(rows['clearance'][:, q]) for q in range(B * A)]
    assert np.array_equal(out['contact_step'], [c for c, _ in outc])
    assert np.array_equal(out['min_clearance'], [m for _, m in outc])
    d = np.hypot(rows['x'] - goal[:, 0], rows['y'] - goal[:, 1])
    print('outcomes: %d of %d egos arrived, %d contacts after separation, worst clearance after separation %.3f m; closest |d - GOAL_DIS| %.2e, '
          '|v - STOP_SPEED| %.2e' % ((want_goal >= 0).sum(), B * A, (out['contact_step'] >= 0).sum(), out['min_clearance'].min(),
                                     np.abs(d - GOAL_DIS).min(), np.abs(np.abs(rows['v']) - STOP_SPEED).min()))


def test_single_ego_and_agent_sharded_layouts(ctx, stock):
    """config2_batch (one ego per instance, no traffic): nobody to measure against, clearance +inf and no contact.  The agent-sharded
    layout on a one-rank communicator (MPCX_SHARD_AGENTS inside the logged closed loop: the pool is the all-gathered one) and with a
    callable exchange (the staged path): the plain batch's log bit for bit.  (The two-process rehearsal of tests/test_gpu_multirank.py
    runs a worker that attaches no log: test_agent_sharded_two_ranks below has a worker of its own.)"""
    from mpc_for_av_at_intersection_amd.batch import config2_batch, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    routes, dl, cd = stock
    solo = config2_batch(ctx, B=64, T=13, seed=4)
    log = solo.attach_log(6)
    solo.run(6)
    rows, out = log.rows(), log.outcomes()
    assert rows.shape == (6, 64) and np.isinf(rows['clearance']).all() and (rows['clearance'] > 0).all()
    assert (out['contact_step'] == -1).all() and np.isinf(out['min_clearance']).all() and (out['steps'] == 6).all()
    assert np.isfinite(rows['xref_deviation'][rows['status'] == 0]).all() and np.isnan(rows['xref_deviation'][rows['status'] != 0]).all()
    plain = synthetic_batch(ctx, B=16, A=8, T=13, seed=5, routes=routes, dl=dl, cd=cd)
    plog = plain.attach_log(5)
    plain.run(5)
    want = plog.rows()
    assert np.isfinite(want['clearance']).all()
    c1 = Context(0)
    c1.comm_init(1, 0, c1.comm_unique_id())
    rccl = synthetic_batch(c1, B=16, A=8, T=13, seed=5, routes=routes, dl=dl, cd=cd, agent_shard=(0, 1), exchange='rccl')
    rlog = rccl.attach_log(5)
    rccl.run(5)
    _assert_rows_equal(rlog.rows(), want, 'rccl')
    c1.comm_destroy()
    c1.close()
    call = synthetic_batch(ctx, B=16, A=8, T=13, seed=5, routes=routes, dl=dl, cd=cd, agent_shard=(0, 1), exchange=lambda loc: loc.clone())
    clog = call.attach_log(5)
    call.run(5)
    _assert_rows_equal(clog.rows(), want, 'callable exchange')


def test_agent_sharded_two_ranks(ctx, stock, tmp_path):
    """agent a of every instance on rank a // 4, two processes sharing the GPU, rows over gloo: each rank's pool is the all-gathered one
    (8 rows per instance, the rank's 4 agents somewhere inside it), so a record stage that read obs_off / obs_skip against the rank's
    own rows would measure the wrong vehicles.  Each rank's log = its agents' part of the single-rank log, bit for bit, the clearance
    and the outcomes included; and the egos do come near each other (clearances of a few metres), so the column is not all far-field."""
    import os
    import torch.multiprocessing as mp
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    from tests import runlog_workers
    routes, dl, cd = stock
    B, steps, seed, world = 12, 10, 7, 2
    plain = synthetic_batch(ctx, B=B, A=8, T=13, seed=seed, routes=routes, dl=dl, cd=cd)
    plog = plain.attach_log(steps)
    plain.run(steps)
    want, wout = plog.rows().reshape(steps, B, 8), plog.outcomes()
    assert np.isfinite(want['clearance']).all() and want['clearance'].min() < 10.0
    mpc = mp.get_context('spawn')
    port = 28000 + os.getpid() % 4000
    out = str(tmp_path / 'runlog_%d.npz')
    procs = [mpc.Process(target=runlog_workers.logged_agent_shard_worker, args=(r, world, port, B, steps, seed, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for r in range(world):
        part = np.load(out % r)
        _assert_rows_equal(part['rows'].reshape(steps, B, 4), want[:, :, 4 * r:4 * r + 4], 'rank %d' % r)
        for k, v in wout.items():
            assert np.array_equal(part[k].reshape(B, 4), v.reshape(B, 8)[:, 4 * r:4 * r + 4]), (r, k)


def test_capacity_rules(ctx, stock):
    """capacity 3, 5 steps: 3 rows, steps = 5, the outcomes of all 5 steps; capacity 0: outcomes only (24 bytes per agent); reset() starts
    over; a log beyond the stated limit is refused unless the caller lifts the limit"""
    full, small, none = _family(ctx, stock), _family(ctx, stock), _family(ctx, stock)
    lf, ls, ln = full.attach_log(40), small.attach_log(3), none.attach_log(0)
    assert ln.nbytes == 24 * none.P and ls.nbytes == 3 * small.P * 96 + 24 * small.P and ln.rows_f64 is None
    for sim in (full, small, none):
        sim.run(40)
    rows = lf.rows()
    assert ls.rows().shape == (3, small.P) and ln.rows().shape == (0, none.P)
    _assert_rows_equal(ls.rows(), rows[:3], 'overflow')
    of = lf.outcomes()
    assert (of['steps'] == 40).all() and np.isfinite(of['min_clearance']).any()
    for other in (ls, ln):
        o = other.outcomes()
        for k in of:
            assert np.array_equal(of[k], o[k]), k
    q = int(np.argmin(of['min_clearance']))
    assert np.array_equal(ls.rows(q), rows[:3, q]) and len(lf.rows(q)) == 40
    lf.reset()
    assert lf.rows().shape == (0, full.P) and (lf.outcomes()['steps'] == 0).all() and np.isinf(lf.outcomes()['min_clearance']).all()
    assert np.array_equal(lf.initial, full.snapshot()['state'])
    full.run(2)
    assert lf.rows().shape == (2, full.P) and np.array_equal(lf.rows()['x'][1], full.snapshot()['state'][:, 0])
    with pytest.raises(ValueError, match='exceed the limit'):
        full.attach_log(1000, max_bytes=1 << 20)
    with pytest.raises(ValueError, match='negative'):
        full.attach_log(-1)
    assert full.attach_log(1000, max_bytes=None).capacity == 1000


def test_refusals(ctx, stock):
    """every invalid log descriptor is MPCX_E_INVALID with a message, from the closed loop and from the per-stage entry point alike, before
    anything is launched: row buffers missing with a capacity, any outcome buffer missing, a negative capacity, goal parameters that are
    not numbers >= 0, and a descriptor without obs_skip (the agent's own pool row is its pose)"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    sim = _family(ctx, stock, B=4)
    log = sim.attach_log(2)
    desc = sim._descriptor()
    before = sim.snapshot()

    def variant(**kw):
        c = _lib.RunLogC()
        C.memmove(C.byref(c), C.byref(log.c), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def staged(c, obs_skip=sim.obs_skip):
        ctx.record_step(sim.ip, sim.state, sim.applied, sim.sol['x'], sim.path, sim.path_off, sim.path_len, sim.target_ind, sim.inter['cut_len'],
                        sim.traj_idx, sim.inter['hit_idx'], sim.sol['status'], sim.sol['iters'], sim.obs6, sim.obs_off, sim.obs_cnt, obs_skip, c)
    bad = [variant(rows_f64=None), variant(rows_i32=None), variant(capacity=-1), variant(goal_dis=float('nan')), variant(stop_speed=-1.0)]
    bad += [variant(**{k: None}) for k in ('steps', 'goal_step', 'contact_step', 'flags', 'min_clearance')]
    for c in bad:
        for graph in (False, True):
            with pytest.raises(MpcxError, match=r'mpcx error -1: run log'):
                ctx.closed_loop_run(sim.ip, desc, 1, graph, log=c)
        with pytest.raises(MpcxError, match=r'mpcx error -1: run log'):
            staged(c)
    no_skip = sim._descriptor()
    no_skip.obs_skip = None
    with pytest.raises(MpcxError, match=r'mpcx error -1: run log: obs_skip'):
        ctx.closed_loop_run(sim.ip, no_skip, 1, log=log.c)
    with pytest.raises(MpcxError, match=r'mpcx error -1: run log: obs_skip'):
        staged(log.c, obs_skip=None)
    # nothing ran, nothing was recorded (bytes: no step has written the solution buffers yet, they hold whatever the allocator left)
    after = sim.snapshot()
    for k, v in before.items():
        assert v.tobytes() == after[k].tobytes(), k
    assert (log.outcomes()['steps'] == 0).all()
    # an all-zero descriptor is "no log": the plain run
    twin = _family(ctx, stock, B=4)
    ctx.closed_loop_run(sim.ip, desc, 2, log=_lib.RunLogC())
    twin.run(2)
    a, b = sim.snapshot(), twin.snapshot()
    for k, v in b.items():
        assert np.array_equal(v, a[k]), k
    assert (log.outcomes()['steps'] == 0).all()
