"""GPU tests of the closed loop's second stop mode (stop_mode='speed'): the reference's newer scenario script,
main/scenarios/mpc_intersection_new_ref.py:90-159 with lib/mpc_with_speed.py -- the path stays whole, the conflict search's cut index is a
per-agent stop index and the speed reference is zeroed from it on.  The recorded run (tests/golden/closedloop_speedref.npz) on the device
alone, run = staged = graph, the oracle replay of a mixed batch (tests/speedref_helpers.agent_step), the run log, the unchanged cut mode,
route_speed and the refusals.  The CPU side is tests/test_speedref_cpu.py."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import speedref_helpers as S

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


def _speed_params(cd):
    import mpc_for_av_at_intersection_amd.lib.mpc_with_speed as ws
    assert ws.T == 13
    return ws.params(cd, 0.2)


def _golden_batch(c, kind, B=8):
    """the recorded scenario, B identical copies: the ego on path (1, 1) and the script's two cars (mpc_intersection_new_ref.py:42-45) as
    tapes of their recorded get() rows or as actors generated on the device"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.lib import moving_obstacles as mo
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, Traffic
    g = H.gold('closedloop_speedref.npz')
    cd = BicycleModelDimensions()
    full = g['full'].copy()
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    if kind == 'tape':
        tr = Traffic.from_tapes([g['obs6']], [0] * B)
    else:
        tr = Traffic.from_objects([[mo.MovingObstacleTIntersection(cd, direction=1, offset=1., turning=False, speed=25 / 3.6, dt=0.2),
                                    mo.MovingObstacleTIntersection(cd, direction=-1, offset=4., turning=True, speed=25 / 3.6, dt=0.2)]
                                   for _ in range(B)])
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(c, _speed_params(cd), ip, [full], dl, np.zeros((B, 1), int), np.zeros((B, 1), int), traffic=tr, stop_mode='speed')


@pytest.mark.parametrize('kind', ['tape', 'generated'])
def test_recorded_speed_reference_closed_loop_on_the_device(ctx, kind):
    """mpc_intersection_new_ref.py:90-159 -- the ego on path (1, 1), its whole path kept, and the script's two cars -- advanced on the device
    alone, 8 identical copies, against the reference's recorded run: traj_agent_idx, hit index, stop index and target_ind exact, state
    before each step and applied controls within 1e-6, every status 0, at least 40 steps with a stop index.  Then the whole run as ONE
    run(n) and as a replayed hipGraph on a side stream: final snapshots bit-identical to the step-by-step run (the length of the
    previous tmp_trajectory is 0 before the first step and the path length afterwards: kept on the host it would be frozen into the graph)."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    g = H.gold('closedloop_speedref.npz')
    n_steps = int(g['steps'])
    B = 8
    sim = _golden_batch(ctx, kind, B)
    assert sim.v_ref == float(g['v_ref']) == S.V_REF
    worst_s = worst_u = 0.0
    n_stop = 0
    for i in range(n_steps):
        before = sim.snapshot()
        assert (before['prev_cut'] == (0 if i == 0 else len(g['full']))).all(), i
        ds = float(np.abs(before['state'] - g['state'][i]).max())
        worst_s = max(worst_s, ds)
        assert ds < 1e-6, (i, ds)
        sim.run(1)
        after = sim.snapshot()
        stop = sim.stop_index()
        want_hit, want_stop = int(g['hit'][i][2]), int(g['stop'][i])
        n_stop += int(want_stop != S.NO_STOP)
        assert (after['traj_idx'] == g['tidx'][i]).all(), (i, after['traj_idx'], g['tidx'][i])
        assert (after['hit_idx'] == want_hit).all(), (i, after['hit_idx'], want_hit)
        assert (stop == want_stop).all(), (i, stop, want_stop)
        assert (after['cut_len'] == (want_stop if want_stop != S.NO_STOP else len(g['full']))).all(), (i, after['cut_len'])
        assert (after['target_ind'] == g['target'][i]).all(), (i, after['target_ind'], g['target'][i])
        assert (after['status'] == 0).all(), i
        assert np.isin(after['xref'][:, 2], (0.0, S.V_REF)).all() and ((after['xref'][0, 2] == 0).any() <= (want_stop != S.NO_STOP)), i
        du = float(np.abs(after['applied'] - g['ctrl'][i]).max())
        worst_u = max(worst_u, du)
        assert du < 1e-6, (i, du)
        for k, v in after.items():          # the 8 copies are one run
            assert np.array_equal(v.reshape((B, -1)), np.repeat(v.reshape((B, -1))[:1], B, axis=0)), (i, k)
    assert n_stop >= 40
    print('speed reference, %s actors: %d steps (%d with a stop index), worst |state - golden| %.2e, worst |control - golden| %.2e'
          % (kind, n_steps, n_stop, worst_s, worst_u))
    final = sim.snapshot()
    one = _golden_batch(ctx, kind, B)
    one.run(n_steps)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    gr = _golden_batch(side, kind, B)
    gr.run(n_steps, graph=True)
    for name, s in (('one call', one.snapshot()), ('graph', gr.snapshot())):
        for k, v in final.items():
            assert np.array_equal(v, s[k]), (name, k)
    side.close()


@pytest.mark.parametrize('lin_passes', [1, 2])
def test_run_equals_staged_equals_graph_in_speed_mode(ctx, stock, lin_passes):
    """scripted_traffic_batch(B = 24, A = 3, K = 2, T = 13, seed = 3, stop_mode = 'speed'), with one and with two linearisation passes per
    step: 10 steps stage by stage, as one run(10) and as graph replays of 4 + 6 steps: every snapshot buffer bit-identical"""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    routes, dl, cd = stock
    side = Context(0, stream=torch.cuda.Stream(device=0))
    sims = {name: scripted_traffic_batch(c, B=24, A=3, K=2, seed=3, routes=routes, dl=dl, cd=cd, mpc=_speed_params(cd), stop_mode='speed')
            for name, c in (('staged', ctx), ('fused', ctx), ('graph', side))}
    for s in sims.values():
        s.lin_passes = lin_passes
    torch.cuda.synchronize()
    for _ in range(10):
        sims['staged'].step_staged()
    sims['fused'].run(10)
    sims['graph'].run(4, graph=True)
    sims['graph'].run(6, graph=True)
    snaps = {k: s.snapshot() for k, s in sims.items()}
    torch.cuda.synchronize()
    ref = snaps['staged']
    plen = sims['staged'].path_len.cpu().numpy()
    assert sims['staged'].A >= 2 and sims['staged'].traffic.k_of_instance.max() == 2 and ref['state'][:, 2].max() > 1.0
    assert np.array_equal(ref['prev_cut'], plen) and (ref['cut_len'] < plen).any() and (ref['cut_len'] == plen).any()
    assert (ref['traffic_state'][:, 3] == 10).all()
    for name in ('fused', 'graph'):
        for key, val in ref.items():
            assert np.array_equal(val, snaps[name][key]), (name, key)
    side.close()


def test_oracle_replay_of_a_mixed_speed_batch(ctx, stock):
    """scripted_traffic_batch(B = 64, A = 2, K = 2, T = 13, seed = 15, stop_mode = 'speed') with the constants of lib/mpc_with_speed.py: 30
    burn-in steps, then 4 steps in which EVERY ego (128 per step) is replayed with the composed oracle step
    (tests/speedref_helpers.agent_step) from the device state before the step and the pool rows the device wrote for it.  Integer
    decisions -- traj_agent_idx, hit index, stop index, target_ind -- and status identical for every ego, solutions within 2e-7
    (helpers.replay_all_on_oracle's bar).  Not vacuous, by the oracle alone: among the replayed ego-steps at least one has its stop index
    inside the reference window (xref[2] holds both v_ref and 0), at least one has no stop, and the mean ego speed is above 1 m/s.
    Seed 15 was chosen by a run of the family on the oracle alone, on the CPU (scripts/speedref_seed_scan.py, seeds 11 .. 28): 69 of its 512
    ego-steps have the stop index inside the window, 87 have no stop, mean ego speed 1.75 m/s -- the fastest of those seeds (every one of
    them passes the three bars; the slowest, seed 27, has 62 / 61 / 1.16 m/s)."""
    import dataclasses
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    from oracle import oracle_py as orc
    routes, dl, cd = stock
    B, A, K, burn, n_check = 64, 2, 2, 30, 4
    sim = scripted_traffic_batch(ctx, B=B, A=A, K=K, seed=15, routes=routes, dl=dl, cd=cd, mpc=_speed_params(cd), stop_mode='speed')
    assert sim.params.T == 13 and tuple(sim.params.Q_v_yaw) == (20.0, 0.5)
    sim.run(burn)
    sim.check()
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    stride = A + K
    worst = 0.0
    inside = none = 0
    speeds = []
    for step in range(burn, burn + n_check):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        stop = sim.stop_index()
        pool = after['obs6'].reshape(B, stride, 6)
        packed = np.column_stack([before['state'], before['applied'][:, 1], before['applied'][:, 0]]).reshape(B, A, 6)
        assert np.array_equal(pool[:, :A], packed)
        assert np.array_equal(before['prev_cut'], ln)
        speeds.append(before['state'][:, 2])
        for p in range(B * A):
            b, a = divmod(p, A)
            own = b * stride + a
            window = [r for r in range(b * stride, (b + 1) * stride) if r != own]
            r = S.agent_step(po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], after['obs6'][window], int(before['traj_idx'][p]),
                             int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius,
                             sim.ip.cutoff_margin, v_ref=sim.v_ref)
            want_hit = -1 if r['hit'] is None else int(r['hit'][2])
            assert (r['traj_idx'], r['stop'], r['target_ind'], want_hit, r['sol'].status) == \
                (after['traj_idx'][p], stop[p], after['target_ind'][p], after['hit_idx'][p], after['status'][p]), (step, p)
            assert after['cut_len'][p] == (r['stop'] if r['hit'] is not None else ln[p]), (step, p)
            assert r['sol'].status == 0
            assert np.array_equal(r['xref'], after['xref'][p]) and np.array_equal(r['re'], after['reaches_end'][p]), (step, p)
            worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
            v2 = r['xref'][2]
            inside += bool((v2 == 0).any() and (v2 == sim.v_ref).any())
            none += r['stop'] == S.NO_STOP
    mean_speed = float(np.mean(speeds))
    print('mixed speed-mode batch: worst |GPU - oracle| %.2e over %d ego-steps; stop index inside the window %d, no stop %d; mean speed %.2f m/s'
          % (worst, n_check * B * A, inside, none, mean_speed))
    assert worst < 2e-7, worst
    assert inside >= 1 and none >= 1 and mean_speed > 1.0, (inside, none, mean_speed)


def test_run_log_of_the_recorded_run(ctx):
    """the run log in speed mode: outcomes() reports the arrival at the golden's last step (is_goal with len(cx) = the whole path,
    lib/mpc_with_speed.py:314-330), history(q) is the recorded run within 1e-6, the cut_len column holds the stop index; and the log of a
    staged run is the same log"""
    g = H.gold('closedloop_speedref.npz')
    n_steps = int(g['steps'])
    sim = _golden_batch(ctx, 'tape', 4)
    log = sim.attach_log(n_steps + 10)
    sim.run(n_steps + 5)
    out = log.outcomes()
    assert (out['goal_step'] == n_steps).all(), out['goal_step']
    assert (out['steps'] == n_steps + 5).all()
    rows = log.rows()
    stop = np.where(rows['hit_idx'][:n_steps, 0] >= 0, rows['cut_len'][:n_steps, 0], S.NO_STOP)
    assert np.array_equal(stop, g['stop']) and np.array_equal(rows['target_ind'][:n_steps, 0], g['target'])
    for q in (0, 3):
        h = log.history(q)
        assert len(h.x) == n_steps + 1
        got = np.column_stack([h.x, h.y, h.v, h.yaw])
        assert np.abs(got[:n_steps] - g['state']).max() < 1e-6
        assert np.abs(np.column_stack([h.delta, h.a])[1:] - g['ctrl']).max() < 1e-6
    staged = _golden_batch(ctx, 'tape', 4)
    slog = staged.attach_log(n_steps + 10)
    for _ in range(n_steps + 5):
        staged.step_staged()
    srows = slog.rows()
    for name in rows.dtype.names:
        assert np.array_equal(rows[name], srows[name], equal_nan=name == 'xref_deviation'), name
    assert all(np.array_equal(v, slog.outcomes()[k]) for k, v in out.items())


def test_cut_mode_is_todays_bits(ctx, stock):
    """stop_mode='cut' is the batch built without the argument: every snapshot buffer bit-identical, fused and staged, with traffic and
    without; and an agent-sharded (RCCL, one rank) speed-mode batch is the plain speed-mode batch"""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    routes, dl, cd = stock
    kw = dict(routes=routes, dl=dl, cd=cd)
    for make in (lambda **k: scripted_traffic_batch(ctx, B=16, A=2, K=2, T=13, seed=4, **kw, **k),
                 lambda **k: synthetic_batch(ctx, B=8, A=8, T=20, seed=6, **kw, **k)):
        plain, cut, staged = make(), make(stop_mode='cut'), make(stop_mode='cut')
        assert plain.prev_len is None and cut.prev_len is None and cut._opts is None
        plain.run(7)
        cut.run(7)
        for _ in range(7):
            staged.step_staged()
        a = plain.snapshot()
        assert (a['cut_len'] < plain.path_len.cpu().numpy()).any()
        for name, s in (('run', cut.snapshot()), ('staged', staged.snapshot())):
            assert set(s) == set(a)
            for k, v in a.items():
                assert np.array_equal(v, s[k]), (name, k)
    speed = synthetic_batch(ctx, B=8, A=8, T=13, seed=6, mpc=_speed_params(cd), stop_mode='speed', **kw)
    speed.run(7)
    want = speed.snapshot()
    assert not np.array_equal(want['state'], a['state'])
    c1 = Context(0)
    c1.comm_init(1, 0, c1.comm_unique_id())
    rccl = synthetic_batch(c1, B=8, A=8, T=13, seed=6, mpc=_speed_params(cd), stop_mode='speed', agent_shard=(0, 1), exchange='rccl', **kw)
    rccl.run(7)
    got = rccl.snapshot()
    for k, v in want.items():
        assert np.array_equal(v, got[k]), ('rccl', k)
    c1.comm_destroy()
    c1.close()


@pytest.mark.parametrize('stop_mode', ['cut', 'speed'])
def test_route_speed_fills_the_speed_profile(ctx, stop_mode):
    """route_speed -> path_v: the speed-window golden cases of mpc_pre.npz (ws13/*: lib/mpc_with_speed.py's window over a path with a
    NON-UNIFORM profile, MAX_SPEED with zeros from a cutoff on) as a batch of single egos, one route and one profile per case, nobody
    else around (no stop index): xref -- row 2, the profile, included -- target_ind and reaches_end of the first step are the reference's,
    bit for bit, fused and staged"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams
    g = H.gold('mpc_pre.npz')
    cd = BicycleModelDimensions()
    full = H.smoothed_path(4, 1)
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    n = len(g['ws13/state'])
    vmax = float(g['ws/MAX_SPEED'])
    routes, speeds = [], []
    for k in range(n):
        cut, cutoff = int(g['ws13/cut'][k]), int(g['ws13/cutoff'][k])
        cv = np.full(cut, vmax)
        if cutoff != 999:
            cv[cutoff:] = 0
        routes.append(full[:cut]); speeds.append(cv)
    assert sum(len(np.unique(v)) > 1 for v in speeds) >= 3
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    for staged in (False, True):
        sim = IntersectionBatch(ctx, _speed_params(cd), ip, routes, dl, np.arange(n)[:, None], g['ws13/start'][:, None], stop_mode=stop_mode,
                                route_speed=speeds, v_ref=1.25)
        sim.state.copy_(ctx.f64(g['ws13/state']))
        sim.step_staged() if staged else sim.run(1)
        s = sim.snapshot()
        assert np.array_equal(s['target_ind'], g['ws13/target_ind'])
        assert np.array_equal(s['xref'], g['ws13/xref']) and np.array_equal(s['reaches_end'], g['ws13/reaches_end'])
        assert (s['xref'][:, 2] == 0).any() and (s['xref'][:, 2] == vmax).any() and not (s['xref'][:, 2] == 1.25).any()


def test_refusals(ctx, stock):
    """an unknown stop mode, a speed reference that is not finite and a route_speed of the wrong length are refused when the batch is
    built; the library refuses the same options with MPCX_E_INVALID, and a stop index without a finite v_ref in the window stage.  Nothing
    is launched: the batch's buffers are as they were"""
    import ctypes
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    routes, dl, cd = stock
    kw = dict(B=2, A=4, T=13, seed=1, routes=routes, dl=dl, cd=cd, mpc=_speed_params(cd))
    with pytest.raises(MpcxError, match='stop_mode'):
        synthetic_batch(ctx, stop_mode='halt', **kw)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(MpcxError, match='v_ref'):
            synthetic_batch(ctx, stop_mode='speed', v_ref=bad, **kw)
    with pytest.raises(ValueError, match='route_speed'):
        synthetic_batch(ctx, stop_mode='speed', route_speed=[np.ones(len(r)) for r in routes[:-1]], **kw)
    with pytest.raises(ValueError, match='route_speed'):
        synthetic_batch(ctx, stop_mode='speed', route_speed=[np.ones(len(r) - 1) for r in routes], **kw)
    sim = synthetic_batch(ctx, stop_mode='speed', **kw)
    sim.run(2)
    before = sim.snapshot()
    desc = sim._descriptor()
    sim._claim_context()
    for opts, what in ((_lib.ClosedLoopOptsC(7, 0, sim.v_ref, sim.prev_len.data_ptr()), 'stop mode'),
                       (_lib.ClosedLoopOptsC(_lib.STOP_SPEED, 0, float('nan'), sim.prev_len.data_ptr()), 'v_ref'),
                       (_lib.ClosedLoopOptsC(_lib.STOP_SPEED, 0, float('-inf'), sim.prev_len.data_ptr()), 'v_ref'),
                       (_lib.ClosedLoopOptsC(_lib.STOP_SPEED, 0, sim.v_ref, None), 'prev_len')):
        for graph in (False, True):
            with pytest.raises(MpcxError, match='mpcx error -1: .*' + what):
                ctx.closed_loop_run(sim.ip, desc, 1, graph, opts=opts)
    with pytest.raises(MpcxError, match='mpcx error -1: .*v_ref'):
        ctx.prepare(sim.state, sim.sol['u'], sim.path, sim.path_off, sim.path_len, sim.dl, sim.target_ind, out=sim.pre,
                    stop_idx=sim.inter['cut_len'], v_ref=float('nan'), len_seen=sim.prev_len)
    after = sim.snapshot()
    for k, v in before.items():
        assert np.array_equal(v, after[k]), k
    assert ctypes.sizeof(_lib.ClosedLoopOptsC) == 24 and _lib.NO_STOP == 999 and _lib.STOP_MODES == {'cut': 0, 'speed': 1}
    sim.run(1)          # ... and the batch goes on
    assert (sim.snapshot()['status'] == 0).all()


def test_stop_index_999_is_no_stop_in_the_window_kernel(ctx):
    """the reference's quirk on the device (mpcx_mpc_prepare_batch_stop): three egos at point 890 of a straight path of 1500 points, v = 6 m/s,
    so that the window reaches to point 1199, with stop indices 998, 999 and 1000.  999 is `cutoff_idx != 999` of lib/mpc_with_speed.py:281:
    nothing is zeroed although the window passes it; 998 and 1000 zero from there on.  Every window is the oracle's for the profile
    speedref_helpers.speed_profile builds, bit for bit, and len_seen receives the path length."""
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from oracle import oracle_py as orc
    dl, n = 0.05, 1500
    full = np.column_stack([np.arange(n) * dl, np.zeros(n), np.zeros(n)])
    stops = np.array([998, S.NO_STOP, 1000], dtype=np.int32)
    B = len(stops)
    ctx.set_mpc_params(_speed_params(BicycleModelDimensions()))
    state = np.tile([full[890, 0], 0.0, 6.0, 0.0], (B, 1))
    tind, seen = ctx.i32(np.full(B, 890)), ctx.i32(np.zeros(B))
    pre = ctx.prepare(ctx.f64(state), None, ctx.f64(full), ctx.i32(np.zeros(B)), ctx.i32(np.full(B, n)), dl, tind, stop_idx=ctx.i32(stops),
                      v_ref=S.V_REF, len_seen=seen)
    ctx.synchronize()
    xref = pre['xref'].cpu().numpy()
    p = S.speed_params(13)
    for b, stop in enumerate(stops):
        want, s, re = orc.calc_ref_trajectory(p, state[b], full[:, 0], full[:, 1], full[:, 2], dl, 890, cv=S.speed_profile(n, int(stop)))
        assert s == int(tind.cpu()[b]) and np.array_equal(xref[b], want) and np.array_equal(pre['reaches_end'].cpu().numpy()[b], re), b
    idx = np.minimum(np.rint(np.cumsum(np.full(14, 6.0 * 0.2)) / dl).astype(int) + int(tind.cpu()[1]), n - 1)
    assert idx.min() < 998 and idx.max() > 1000
    assert (xref[1, 2] == S.V_REF).all()
    assert np.array_equal(xref[0, 2], np.where(idx >= 998, 0.0, S.V_REF)) and np.array_equal(xref[2, 2], np.where(idx >= 1000, 0.0, S.V_REF))
    assert (xref[0, 2] == 0).any() and (xref[2, 2] == 0).any() and (seen.cpu().numpy() == n).all()
