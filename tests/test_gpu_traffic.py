"""GPU tests of the scripted traffic in the device-resident closed loop: traffic_kernel against the host classes, the reference's
recorded stock scenario (one ego + two scripted cars, tests/golden/closedloop.npz) advanced on the device without the host, run = staged
= graph with traffic, the oracle replay of a mixed batch, the unchanged ego-only path and the refusals.  The host build of the same
step rule is tests/test_traffic_cpu.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_traffic_cpu import golden_vehicles

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-11        # device sincos / tan against numpy's: see test_device_actors_against_host_tapes


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


def _host_tape(obj, n):
    with contextlib.redirect_stdout(io.StringIO()):         # (the roundabout class prints while it turns)
        return obj.tape(n)


def _random_vehicles(n=256, seed=2024):
    from mpc_for_av_at_intersection_amd.lib import moving_obstacles as mo
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    bic = BicycleModelDimensions()
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        speed = rng.uniform(10.0, 35.0) / 3.6
        offset = None if rng.random() < 0.25 else rng.uniform(0.0, 6.0)
        direction = 1 if rng.random() < 0.5 else -1
        turning = bool(rng.random() < 0.6)
        x0, y0 = rng.uniform(-4.0, 4.0), rng.uniform(-40.0, -10.0)
        dt = (0.2, 0.1)[(i // 3) % 2]
        if i % 3 == 0:
            out.append(mo.MovingObstacleTIntersection(bic, direction=direction, turning=turning, speed=speed, offset=offset, dt=dt))
        elif i % 3 == 1:
            out.append(mo.MovingObstacleRoundabout(bic, direction=direction, turning=turning, speed=speed, offset=offset, dt=dt))
        else:
            out.append(mo.MovingObstacleArterial(bic, x_init=x0, y_init=y0, speed=speed, offset=offset, dt=dt))
    return out


def _upload(ctx, tr):
    actors = torch.as_tensor(np.frombuffer(tr.actors.tobytes(), dtype=np.uint8).copy()).to(ctx.device)
    return actors, ctx.f64(tr.state), None if tr.tape is None else ctx.f64(tr.tape)


def test_device_actors_against_host_tapes(ctx):
    """mpcx_traffic_step_batch 150 times on the 36 golden configurations + 256 seeded random vehicles against tape(150) of the host classes.
    Decision columns v, a, steer: identical for every actor and step.  Poses x, y, yaw: within 1e-11 -- the device's sincos / tan may
    differ from numpy's in the last bits; perturbing every trig result of the host classes by up to +-2 ulp moved the poses of these
    very configurations by at most 6.3e-13 and changed no decision, 1e-11 leaves a margin of 16 for a libm that was not measured.
    TAPE actors replay their uploaded rows bit for bit and hold the last one."""
    from mpc_for_av_at_intersection_amd.runtime import Traffic
    n_steps = 150
    objs = [o for _, o, _ in golden_vehicles()] + _random_vehicles()
    assert len(objs) == 36 + 256
    tr = Traffic.from_objects([objs])
    want = np.stack([_host_tape(o, n_steps) for o in objs], axis=1)           # (steps, actors, 6)
    actors, state, _ = _upload(ctx, tr)
    n = tr.n_actors
    rows = ctx.i32(np.arange(n)[::-1].copy())                                 # any permutation of the pool will do
    obs6 = torch.zeros((n, 6), dtype=torch.float64, device=ctx.device)
    got = np.zeros_like(want)
    for k in range(n_steps):
        ctx.traffic_step(actors, state, rows, obs6)
        ctx.synchronize()
        got[k] = obs6.cpu().numpy()[::-1]
    for col, name in ((2, 'v'), (4, 'a'), (5, 'steer')):
        bad = np.argwhere(got[:, :, col] != want[:, :, col])
        assert len(bad) == 0, '%s differs for %d (step, actor) pairs, first %s' % (name, len(bad), bad[:4].tolist())
    worst = float(np.abs(got[:, :, [0, 1, 3]] - want[:, :, [0, 1, 3]]).max())
    print('device actors vs host classes: %d actors x %d steps, worst pose deviation %.3e' % (n, n_steps, worst))
    assert worst <= POSE_TOL, worst
    assert (np.ptp(want[:, :, 3], axis=0) > 1.0).sum() >= 40                  # the turning branches really turn
    final = state.cpu().numpy()
    assert np.array_equal(final[:, 3], np.full(n, float(n_steps)))
    # TAPE actors
    rng = np.random.default_rng(7)
    tracks = [rng.normal(size=(150, 3, 6)), rng.normal(size=(40, 2, 6))]
    tp = Traffic.from_tapes(tracks, [0, 1, 1, 0])
    actors, state, tape = _upload(ctx, tp)
    m = tp.n_actors
    rows = ctx.i32(np.arange(m))
    obs6 = torch.zeros((m + 2, 6), dtype=torch.float64, device=ctx.device)
    src = [tracks[0][:, 0], tracks[0][:, 1], tracks[0][:, 2], tracks[1][:, 0], tracks[1][:, 1], tracks[1][:, 0], tracks[1][:, 1],
           tracks[0][:, 0], tracks[0][:, 1], tracks[0][:, 2]]
    for k in range(60):
        ctx.traffic_step(actors, state, rows, obs6, tape=tape)
        ctx.synchronize()
        out = obs6.cpu().numpy()
        for i in range(m):
            assert np.array_equal(out[i], src[i][min(k, len(src[i]) - 1)]), (k, i)
        assert not out[m:].any()


def _ego_batch(c, stock, B, A, T, seed, traffic, **kw):
    """IntersectionBatch from the arguments synthetic_batch(c, B, A, T, seed) draws (one agent per route, seeded start indices), + traffic"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, MpcParams
    routes, dl, cd = stock
    rng = np.random.default_rng(seed)
    route_of_agent = np.tile(np.arange(A) % len(routes), (B, 1))
    lens = np.array([len(r) for r in routes])[route_of_agent]
    start = (rng.random((B, A)) * 0.35 * lens).astype(np.int64)
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(c, MpcParams(T=T, L=cd.distance_back_to_front_wheel), ip, routes, dl, route_of_agent, start, traffic=traffic, **kw)


def test_straight_cars_are_bit_identical_on_the_device(ctx):
    """A vehicle whose heading stays 0 -- T-intersection and roundabout cars from the left that do not turn -- meets cos(0) = 1, sin(0) = 0
    and tan(0) = 0 in every math library, so nothing but the rule's own products and sums (x + (v * 1) * dt, each rounded on its own)
    decides its poses: all six columns must equal the host classes' tapes BIT FOR BIT.  A build that contracts x + dx * dt into a fused
    multiply-add rounds once where the classes round twice and fails here (the host build of the rule compiled with contraction on
    differs from these very tapes for 220 of the 256 vehicles), whatever the pose tolerance of the test above would forgive."""
    from mpc_for_av_at_intersection_amd.lib import moving_obstacles as mo
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from mpc_for_av_at_intersection_amd.runtime import Traffic
    bic = BicycleModelDimensions()
    rng = np.random.default_rng(31)
    objs = []
    for i in range(256):
        cls = (mo.MovingObstacleTIntersection, mo.MovingObstacleRoundabout)[i % 2]
        objs.append(cls(bic, direction=1, turning=False, speed=rng.uniform(10.0, 35.0) / 3.6,
                        offset=None if i % 4 == 3 else rng.uniform(0.0, 6.0), dt=(0.2, 0.1, 0.05)[i % 3]))
    tr = Traffic.from_objects([objs])
    want = np.stack([_host_tape(o, 150) for o in objs], axis=1)
    assert (want[:, :, 3] == 0.0).all() and (want[-1, :, 0] > want[0, :, 0] + 5.0).all()
    actors, state, _ = _upload(ctx, tr)
    rows = ctx.i32(np.arange(256))
    obs6 = torch.zeros((256, 6), dtype=torch.float64, device=ctx.device)
    for k in range(150):
        ctx.traffic_step(actors, state, rows, obs6)
        ctx.synchronize()
        got = obs6.cpu().numpy()
        bad = np.nonzero((got != want[k]).any(axis=1))[0]
        assert len(bad) == 0, 'step %d: %d vehicles differ from the host classes, first %s: %s vs %s' % (k, len(bad), bad[:3], got[bad[0]], want[k][bad[0]])


def _stock_batch(c, T, kind, B=8):
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, MpcParams, Traffic
    cd = BicycleModelDimensions()
    full = H.smoothed_path(4, 1)
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    if kind == 'tape':
        tr = Traffic.from_tapes([H.gold('moving.npz')['traffic/tape']], [0] * B)
    else:
        tr = Traffic.from_objects([[o for n, o, _ in golden_vehicles() if n.startswith('stock')] for _ in range(B)])
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(c, MpcParams(T=T, L=cd.distance_back_to_front_wheel), ip, [full], dl, np.zeros((B, 1), int), np.zeros((B, 1), int),
                             traffic=tr), full


@pytest.mark.parametrize('kind', ['tape', 'generated'])
@pytest.mark.parametrize('T', [10, 13, 20])
def test_recorded_stock_closed_loop_on_the_device(ctx, T, kind):
    """main/scenarios/mpc_intersection.py:95-159 -- the ego on path (4, 1) and the two scripted cars of :42-45 -- advanced on the device
    alone, 8 identical copies, against the reference's recorded run (closedloop.npz): integer decisions exact, state before each step and
    applied controls within 1e-6 (the bars of test_stock_closed_loop_matches_reference_run, which drives the same golden through the
    host classes).  Then the whole run as ONE run(n) and as a replayed hipGraph on a side stream: final snapshots bit-identical to the
    step-by-step run (a step counter kept on the host would replay step 0 for ever)."""
    from mpc_for_av_at_intersection_amd.runtime import Context
    g = H.gold('closedloop.npz')
    pre = 'T%d/' % T
    n_steps = int(g[pre + 'steps'])
    B = 8
    sim, full = _stock_batch(ctx, T, kind, B)
    assert np.array_equal(full, g[pre + 'full'])
    worst_s = worst_u = 0.0
    n_hit = 0
    for i in range(n_steps):
        before = sim.snapshot()
        ds = float(np.abs(before['state'] - g[pre + 'state'][i]).max())
        worst_s = max(worst_s, ds)
        assert ds < 1e-6, (i, ds)
        sim.run(1)
        after = sim.snapshot()
        hit = g[pre + 'hit'][i][2]
        want_hit = int(hit) if hit >= 0 else -1
        n_hit += int(want_hit >= 0)
        assert (after['traj_idx'] == g[pre + 'tidx'][i]).all(), (i, after['traj_idx'], g[pre + 'tidx'][i])
        assert (after['hit_idx'] == want_hit).all(), (i, after['hit_idx'], want_hit)
        assert (after['cut_len'] == g[pre + 'cut'][i]).all(), (i, after['cut_len'], g[pre + 'cut'][i])
        assert (after['target_ind'] == g[pre + 'target'][i]).all(), (i, after['target_ind'], g[pre + 'target'][i])
        assert (after['status'] == 0).all(), i
        du = float(np.abs(after['applied'] - g[pre + 'ctrl'][i]).max())
        worst_u = max(worst_u, du)
        assert du < 1e-6, (i, du)
        for k, v in after.items():          # the 8 copies are one run
            assert np.array_equal(v.reshape((B, -1)), np.repeat(v.reshape((B, -1))[:1], B, axis=0)), (i, k)
    assert n_hit >= 60
    print('T=%d %s actors: %d steps (%d with a conflict), worst |state - golden| %.2e, worst |control - golden| %.2e'
          % (T, kind, n_steps, n_hit, worst_s, worst_u))
    final = sim.snapshot()
    one, _ = _stock_batch(ctx, T, kind, B)
    one.run(n_steps)
    side = Context(0, stream=torch.cuda.Stream(device=0))
    gr, _ = _stock_batch(side, T, kind, B)
    gr.run(n_steps, graph=True)
    for name, s in (('one call', one.snapshot()), ('graph', gr.snapshot())):
        for k, v in final.items():
            assert np.array_equal(v, s[k]), (name, k)
    side.close()


def test_run_equals_staged_equals_graph_with_traffic(ctx, stock):
    """scripted_traffic_batch(B = 24, A = 3, K = 2, T = 13, seed = 3): 6 steps stage by stage, as one run(6) and as graph replays of 2 + 4
    steps: every snapshot buffer, the actors' states and the pool rows included, bit-identical"""
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    routes, dl, cd = stock
    side = Context(0, stream=torch.cuda.Stream(device=0))
    sims = {name: scripted_traffic_batch(c, B=24, A=3, K=2, T=13, seed=3, routes=routes, dl=dl, cd=cd)
            for name, c in (('staged', ctx), ('fused', ctx), ('graph', side))}
    torch.cuda.synchronize()
    for _ in range(6):
        sims['staged'].step_staged()
    sims['fused'].run(6)
    sims['graph'].run(2, graph=True)
    sims['graph'].run(4, graph=True)
    snaps = {k: s.snapshot() for k, s in sims.items()}
    torch.cuda.synchronize()
    ref = snaps['staged']
    assert 'traffic_state' in ref and 'obs6' in ref and ref['obs6'].shape == (24 * 5, 6)
    assert (ref['status'] == 0).all() and ref['state'][:, 2].max() > 1.0
    assert (ref['traffic_state'][:, 3] == 6).all() and np.abs(ref['obs6'].reshape(24, 5, 6)[:, 3:, 2]).max() > 1.0     # the cars have started
    for name in ('fused', 'graph'):
        for key, val in ref.items():
            assert np.array_equal(val, snaps[name][key]), (name, key)
    side.close()


def _replay(po, sim, before, after, tab, off, ln, p, rows):
    from oracle import oracle_py as orc
    return orc.agent_step(po, tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], after['obs6'][rows], int(before['traj_idx'][p]),
                          int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p],
                          np.asarray(sim.ip.circle_centers).reshape(2, 2), sim.ip.radius, sim.ip.cutoff_margin)


def test_oracle_replay_of_a_mixed_batch(ctx, stock):
    """scripted_traffic_batch(B = 64, A = 2, K = 2, T = 20, seed = 22): 30 burn-in steps, then 4 steps in which EVERY ego (128 per step) is
    replayed with oracle_py.agent_step.  (Seed 22, not 11: six seconds into the run most egos of this family stand at a path cut in front
    of a crossing car -- with seed 11 the mean ego speed over the four steps is 0.69 m/s, on the device and in a run of the same family
    on the oracle alone, which misses the not-vacuous bar below; the oracle-only run gives 1.16 m/s for seed 22, the fastest of seeds
    11 .. 28.  The bar itself stays.)  The obstacles of a step are the rows of the ego's pool window except its own AS THE DEVICE WROTE
    THEM FOR THAT STEP: the pool is filled at the start of a step and not touched again, so they are read from the snapshot taken after
    it, and checked there against their sources -- the agents' rows against the state and applied controls of the snapshot before, the
    actors' rows against the host classes' tapes.  Integer decisions and status identical for every ego, solutions within 2e-7
    (helpers.replay_all_on_oracle's bar).  Not vacuous, by the oracle alone: at least one ego has a conflict with ONLY the scripted cars
    in its obstacle list, at least one with ONLY the other egos, and the egos move (mean speed above 1 m/s)."""
    import dataclasses
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, scripted_traffic_specs
    from mpc_for_av_at_intersection_amd.lib import moving_obstacles as mo
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    from oracle import oracle_py as orc
    routes, dl, cd = stock
    B, A, K, burn, n_check = 64, 2, 2, 30, 4
    sim = scripted_traffic_batch(ctx, B=B, A=A, K=K, T=20, seed=22, routes=routes, dl=dl, cd=cd)
    spec = scripted_traffic_specs(B, K, 22, cd.distance_back_to_front_wheel)
    bic = BicycleModelDimensions()
    tapes = np.stack([_host_tape(mo.MovingObstacleTIntersection(bic, direction=int(a['direction']), turning=bool(a['turning']),
                                                                  speed=float(a['speed']), offset=float(a['offset']), dt=0.2), burn + n_check)
                      for a in spec.actors], axis=1)                               # (steps, B * K, 6)
    sim.run(burn)
    sim.check()
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    stride = A + K
    worst = 0.0
    by_cars = by_egos = 0
    speeds = []
    for step in range(burn, burn + n_check):
        before = sim.snapshot()
        sim.run(1)
        after = sim.snapshot()
        pool = after['obs6'].reshape(B, stride, 6)
        packed = np.column_stack([before['state'], before['applied'][:, 1], before['applied'][:, 0]]).reshape(B, A, 6)
        assert np.array_equal(pool[:, :A], packed)
        cars = tapes[step].reshape(B, K, 6)
        assert np.array_equal(pool[:, A:, [2, 4, 5]], cars[:, :, [2, 4, 5]]) and np.abs(pool[:, A:] - cars).max() <= POSE_TOL
        speeds.append(before['state'][:, 2])
        for p in range(B * A):
            b, a = divmod(p, A)
            own = b * stride + a
            window = [r for r in range(b * stride, (b + 1) * stride) if r != own]
            r = _replay(po, sim, before, after, tab, off, ln, p, window)
            want_hit = -1 if r['hit'] is None else int(r['hit'][2])
            assert (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status) == \
                (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p]), (step, p)
            assert r['sol'].status == 0
            worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
            if want_hit >= 0:
                by_cars += _replay(po, sim, before, after, tab, off, ln, p, [w for w in window if w >= b * stride + A])['hit'] is not None
                by_egos += _replay(po, sim, before, after, tab, off, ln, p, [w for w in window if w < b * stride + A])['hit'] is not None
    mean_speed = float(np.mean(speeds))
    print('mixed batch: worst |GPU - oracle| %.2e over %d ego-steps; conflicts with only the cars %d, with only the egos %d; mean speed %.2f m/s'
          % (worst, n_check * B * A, by_cars, by_egos, mean_speed))
    assert worst < 2e-7, worst
    assert by_cars >= 1 and by_egos >= 1 and mean_speed > 1.0, (by_cars, by_egos, mean_speed)


def test_no_traffic_is_todays_bits(ctx, stock):
    """an empty Traffic (K = 0 everywhere) takes the ego-only path: every buffer of the plain batch's snapshot bit-identical"""
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Traffic
    routes, dl, cd = stock
    plain = synthetic_batch(ctx, B=16, A=8, T=13, seed=5, routes=routes, dl=dl, cd=cd)
    empty = _ego_batch(ctx, stock, 16, 8, 13, 5, Traffic.empty(16))
    staged = _ego_batch(ctx, stock, 16, 8, 13, 5, Traffic.empty(16))
    plain.run(5)
    empty.run(5)
    for _ in range(5):
        staged.step_staged()
    a = plain.snapshot()
    assert 'traffic_state' not in a and 'obs6' not in a
    for name, s in (('run', empty.snapshot()), ('staged', staged.snapshot())):
        assert s['traffic_state'].shape == (0, 4) and s['obs6'].shape == (16 * 8, 6)
        for k, v in a.items():
            assert np.array_equal(v, s[k]), (name, k)
    assert np.array_equal(empty.snapshot()['obs6'], plain.obs6.cpu().numpy())


def test_refusals(ctx, stock):
    """traffic in the agent-sharded (RCCL) layout and a TAPE actor without a table are refused with MPCX_E_INVALID and a message; more
    than MPCX_MAX_OBS moving obstacles per ego is a ValueError when the batch is built"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_specs
    from mpc_for_av_at_intersection_amd.runtime import Context, MpcxError, Traffic
    routes, dl, cd = stock
    L = cd.distance_back_to_front_wheel
    c1 = Context(0)
    c1.comm_init(1, 0, c1.comm_unique_id())
    sim = _ego_batch(c1, stock, 4, 8, 13, 1, scripted_traffic_specs(4, 2, 1, L), agent_shard=(0, 1), exchange='rccl')
    with pytest.raises(MpcxError, match='agent-sharded'):
        sim.run(1)
    with pytest.raises(MpcxError, match='agent-sharded'):
        sim.step_staged()
    c1.comm_destroy()
    c1.close()
    with pytest.raises(ValueError, match='by instances'):
        _ego_batch(ctx, stock, 4, 8, 13, 1, scripted_traffic_specs(4, 2, 1, L), agent_shard=(0, 2), exchange='rccl')
    with pytest.raises(ValueError, match='MPCX_MAX_OBS'):
        _ego_batch(ctx, stock, 4, 8, 13, 1, scripted_traffic_specs(4, 10, 1, L))
    # a TAPE actor and no table
    tp = Traffic.from_tapes([np.zeros((5, 1, 6))], [0, 0])
    actors, state, _ = _upload(ctx, tp)
    rows = ctx.i32(np.arange(2))
    obs6 = torch.zeros((2, 6), dtype=torch.float64, device=ctx.device)
    with pytest.raises(MpcxError, match=r'mpcx error -1: .*TAPE'):
        ctx.traffic_step(actors, state, rows, obs6, tape=None)
    with pytest.raises(MpcxError, match='mpcx error -1'):       # ... or a table the tape leaves
        ctx.traffic_step(actors, state, rows, obs6, tape=torch.zeros((3, 6), dtype=torch.float64, device=ctx.device))
    with pytest.raises(MpcxError, match='mpcx error -1'):       # ... or a pool row outside the pool
        ctx.traffic_step(actors, state, ctx.i32([0, 2]), obs6, tape=ctx.f64(tp.tape))
    tp.tape = None
    sim = _ego_batch(ctx, stock, 2, 2, 13, 1, tp)
    with pytest.raises(MpcxError, match=r'mpcx error -1: .*TAPE'):
        sim.run(1)
    assert _lib.TRAFFIC_TAPE == 3
