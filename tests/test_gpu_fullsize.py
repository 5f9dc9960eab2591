"""GPU tests at BASELINE.json's full sizes, through size-independent properties (the oracle only checks samples):
batch = 4096 instances x 8 agents at N = 20 for the MPC step, 2^20 nodes for the expansion."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def test_full_batch_closed_loop_properties(ctx):
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from oracle import oracle_py as orc
    routes, dl, cd = stock_routes(ctx)
    B, A, T = 4096, 8, 20
    sim = synthetic_batch(ctx, B=B, A=A, T=T, seed=7, routes=routes, dl=dl, cd=cd)
    # instance B-1 is made an exact copy of instance 0: identical inputs must give bit-identical outputs wherever they run
    for name in ('state', 'traj_idx', 'target_ind'):
        t = getattr(sim, name)
        t[(B - 1) * A:] = t[:A]
    for _ in range(4):
        sim.step()
    before = sim.snapshot()
    sim.step()
    after = sim.snapshot()
    P = B * A
    st = after['status']
    ok = st == 0                                           # failed solves (if any) are checked one by one against the oracle below
    # 1. every accepted solution is feasible for the bounds of mpc.py:184-191 and satisfies the initial condition
    u, x = after['u'], after['x']
    p = sim.params
    assert (u[ok, 0] <= p.max_accel + 1e-7).all() and (u[ok, 0] >= p.max_decel - 1e-7).all()
    assert (np.abs(u[ok, 1]) <= p.max_steer + 1e-7).all()
    assert (np.abs(np.diff(u[ok, 1], axis=1)) <= p.max_dsteer * p.dt + 1e-7).all()
    assert (x[ok, 2] <= p.max_speed + 1e-7).all() and (x[ok, 2] >= p.min_speed - 1e-7).all()
    assert np.abs(x[ok, :, 0] - before['state'][ok][:, [0, 1, 2, 3]]).max() == 0.0
    # 2. the linear prediction is consistent with its own controls: v_t = v_0 + dt * cumsum(a)
    v_pred = x[ok, 2, 0][:, None] + p.dt * np.cumsum(u[ok, 0], axis=1)
    assert np.abs(v_pred - x[ok, 2, 1:]).max() < 1e-10
    # 3. KKT residuals reported by the kernel (relative stationarity / primal, mean complementarity)
    kkt = after['kkt'][ok]
    assert kkt[:, 1].max() < 1e-7 and kkt[:, 2].max() < 1e-7
    # 4. duplicated instance: bit-identical
    for name in ('u', 'x', 'state', 'cut_len', 'hit_idx', 'traj_idx', 'target_ind', 'status', 'iters'):
        assert np.array_equal(after[name][:A], after[name][(B - 1) * A:]), name
    # 5. structural invariants of the interaction stage
    assert (after['traj_idx'] >= before['traj_idx']).all()                      # path index never moves backwards
    ln = sim.path_len.cpu().numpy()
    assert ((after['cut_len'] > after['traj_idx']) & (after['cut_len'] <= ln)).all()
    # a conflict cuts the path; the only exception is a conflict so close to the end of the path that cut = idx - margin
    # cannot happen any more: none here (and every hit_idx / cut_len is compared with the oracle's below)
    conflict, cut = after['hit_idx'] >= 0, after['cut_len'] < ln
    assert not (cut & ~conflict).any()
    late = conflict & ~cut
    assert (after['traj_idx'][late] + 1 >= ln[late]).all(), int(late.sum())
    # 6. ALL 32768 agents replayed on the oracle from the same inputs: identical decisions and statuses, solutions <= 2e-7
    worst, it_diff, failed = H.replay_all_on_oracle(sim, before, after)
    print('4096 x 8 agents vs oracle: worst %.2e, %d agents with a different iteration count, %d failed solves (same on both sides)' % (worst, it_diff, failed))
    assert it_diff <= P // 1000, it_diff       # (observed since the polish: 0)


def test_config3_1024_instances_8_agents(ctx):
    """BASELINE configs[2] at exactly its size: 8-agent coupled intersection, batch = 1024, N = 20, interaction on-device.
    12 closed-loop steps; after each of the last 4, EVERY agent is replayed on the oracle."""
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    routes, dl, cd = stock_routes(ctx)
    sim = synthetic_batch(ctx, B=1024, A=8, T=20, seed=3, routes=routes, dl=dl, cd=cd)
    sim.run(8)
    worst = 0.0
    before = sim.snapshot()
    for _ in range(4):
        sim.step()
        after = sim.snapshot()
        w, it_diff, failed = H.replay_all_on_oracle(sim, before, after)
        worst = max(worst, w)
        assert it_diff <= 8
        before = after
    sim.check()
    assert (after['hit_idx'] >= 0).mean() > 0.05           # the coupling is exercised: conflicts do occur
    print('1024 x 8: worst |GPU - oracle| = %.2e' % worst)


def test_prius_mpc_refinement_of_prius_paths(ctx):
    """BASELINE configs[4], second half: MPC refinement of the paths the Prius-primitive A* finds on the stock intersection,
    with PriusDimensions (L = 4.0, radius 1.4425, disc centres 3.4 / 0.6; car_dimensions.py:93-107) in every kernel: single-ego
    instances (one per path), 40 closed-loop steps, every step of every agent replayed on the oracle with the same dimensions."""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import PriusDimensions
    from mpc_for_av_at_intersection_amd.lib.motion_primitive import load_motion_primitives
    from mpc_for_av_at_intersection_amd.lib.motion_primitive_search_modified import MotionPrimitiveSearch
    from mpc_for_av_at_intersection_amd.lib.mpc import smooth_yaw
    from mpc_for_av_at_intersection_amd.lib.scenario import intersection
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, MpcParams
    cd = PriusDimensions()
    assert cd.distance_back_to_front_wheel == 4.0
    mps = load_motion_primitives('prius')
    routes = []
    for sp in (1, 2, 3, 4):
        for ti in (1, 2, 3):
            try:
                _, _, traj = MotionPrimitiveSearch(intersection(start_pos=sp, turn_indicator=ti), cd, mps, margin=cd.radius, ctx=ctx).run()
            except Exception as e:                 # the Prius primitive set cannot make every manoeuvre
                assert 'No solution found' in str(e)
                continue
            traj = np.ascontiguousarray(traj)
            smooth_yaw(traj[:, 2])
            routes.append(traj)
    assert len(routes) >= 6, len(routes)
    g = H.gold('astar_runs.npz')
    assert any(len(r) == len(g['mod_pri_4_1/traj']) and np.abs(r[:, :2] - g['mod_pri_4_1/traj'][:, :2]).max() < 1e-9 for r in routes)
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    # the Prius primitives are short: point spacing differs per primitive, use the spacing of each path's first edge like the scripts do
    params = MpcParams(T=20, L=cd.distance_back_to_front_wheel)
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    n = len(routes)
    sim = IntersectionBatch(ctx, params, ip, routes, dl, np.arange(n).reshape(n, 1), np.zeros((n, 1), dtype=np.int64))
    worst, raised_total, dead, alive_steps = 0.0, 0, np.zeros(n, bool), np.zeros(n, int)
    before = sim.snapshot()
    for step in range(40):
        sim.step()
        after = sim.snapshot()
        w, it_diff, failed = H.replay_all_on_oracle(sim, before, after, threads=4, dead=dead)
        worst = max(worst, w)
        raised_total += int(sim.raised.sum())
        dead |= sim.raised
        alive_steps += ~dead
        if dead.any():                          # batch.check() raises where the reference would have raised
            with pytest.raises(Exception, match='something wrong'):
                sim.check()
        else:
            sim.check()
        before = after
    # The Prius primitives have very uneven point spacing (0.09 .. 2.5 m per 61 points), so sooner or later the
    # three path points nearest to the car are not contiguous and the REFERENCE raises Exception('something wrong')
    # (trajectories.py:120; it never runs its MPC on Prius paths itself).  Up to that step every agent-step equals the
    # oracle's, and the step that raises is flagged identically on both sides (hit_idx -3 / batch.check()).
    print('Prius MPC refinement: %d paths, agent-steps checked before the reference raises: %s (total %d), raised: %d' % (n, alive_steps.tolist(), alive_steps.sum(), raised_total))
    assert alive_steps.min() >= 4 and alive_steps.sum() >= 8 * n
    print('Prius MPC refinement: %d paths x 40 steps, worst |GPU - oracle| = %.2e' % (n, worst))


def test_long_closed_loop_stays_exact_against_the_oracle(ctx):
    """150 closed-loop steps of 256 instances x 8 agents -- well into the state the benchmark's steady-state leg runs in: paths cut in
    front of standing egos, cuts that move or are lifted, egos that do not advance (so the window selection has no nearest-index hint from
    the conflict search), conflicts far down the path -- with EVERY agent of six steps along the way replayed on the oracle from the device
    state: path indices, cut lengths, conflict indices and solver statuses identical, solutions within one 2e-7.  (Round 4 changed how
    the conflict search resamples, searches and hands its nearest index to the window selection; the short full-size test above sees the
    start-up phase only.)"""
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    routes, dl, cd = stock_routes(ctx)
    sim = synthetic_batch(ctx, B=256, A=8, T=20, seed=21, routes=routes, dl=dl, cd=cd)
    worst, seen = 0.0, dict(cut=0, standing=0, free=0, moved=0)
    done = 0
    for upto in (12, 30, 55, 80, 115, 149):
        sim.run(upto - done)
        done = upto
        before = sim.snapshot()
        sim.step(); done += 1
        after = sim.snapshot()
        w, it_diff, failed = H.replay_all_on_oracle(sim, before, after, threads=8)
        assert failed == 0 and it_diff <= 4
        worst = max(worst, w)
        seen['cut'] += int((after['cut_len'] < sim.path_len.cpu().numpy()).sum())
        seen['standing'] += int((after['traj_idx'] == before['traj_idx']).sum())
        seen['free'] += int((after['hit_idx'] == -1).sum())
        seen['moved'] += int((after['cut_len'] != before['prev_cut']).sum()) if 'prev_cut' in before else 0
    sim.check()
    print('long closed loop: 6 x 2048 agents replayed, worst |GPU - oracle| %.2e; agent-steps with a cut path %d, standing %d, conflict-free %d'
          % (worst, seen['cut'], seen['standing'], seen['free']))
    assert seen['cut'] > 2000 and seen['standing'] > 500 and seen['free'] > 200


def test_expansion_one_million_nodes(ctx):
    """Config 5 shape: 2^20 frontier nodes, Prius primitives, stock intersection: permutation equivariance, agreement of a
    sample with the oracle, and agreement with the golden nodes embedded in the frontier."""
    from oracle import oracle_py as orc
    tables = H.search_tables('prius', 'int_2_1')
    model = ctx.search_model(*tables)
    om = orc.SearchModel(*tables)
    ex = H.gold('expand.npz')
    rng = np.random.default_rng(0)
    n = 1 << 20
    nodes = np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-np.pi, np.pi, n)])
    gold_nodes = ex['pri/nodes']
    nodes[:len(gold_nodes)] = gold_nodes
    dev = ctx.f64(nodes)
    out = ctx.expand(model, dev)
    perm = rng.permutation(n)
    out_p = ctx.expand(model, ctx.f64(nodes[perm]))
    ctx.synchronize()
    col = out['collide'].cpu().numpy(); nbr = out['nbr'].cpu().numpy()
    assert np.array_equal(col[perm], out_p['collide'].cpu().numpy())            # order of nodes is irrelevant
    assert np.array_equal(nbr[perm], out_p['nbr'].cpu().numpy())
    assert np.array_equal(col[:len(gold_nodes)], ex['pri/collide'])             # reference's flags on its own nodes
    assert np.abs(nbr[:len(gold_nodes)] - ex['pri/nbr']).max() < 1e-12
    idx = rng.choice(n, 4096, replace=False)
    onbr, ocol = orc.expand(om, nodes[idx], host_trig=False)
    assert np.array_equal(ocol, col[idx]) and np.abs(onbr - nbr[idx]).max() < 1e-12
    assert 0.05 < 1.0 - col.mean() < 0.9                                        # both outcomes occur
    # the bulk kernel (>= 4096 nodes: the wavefront works its (record, obstacle) pairs off together, record boxes from the template's box)
    # against the per-lane kernel of the small launches (exact point boxes): the same records, bit for bit
    cost = out['cost'].cpu().numpy()
    for lo in list(range(0, 160000, 4000)) + [n - 4000]:
        part = ctx.expand(model, dev[lo:lo + 4000].contiguous())
        assert np.array_equal(part['collide'].cpu().numpy(), col[lo:lo + 4000]) and np.array_equal(part['nbr'].cpu().numpy(), nbr[lo:lo + 4000])
        assert np.array_equal(part['cost'].cpu().numpy(), cost[lo:lo + 4000])
    # throughput, for the record (not asserted)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        ctx.expand(model, dev, out=out)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    print('expand_kernel: 2^20 nodes x %d primitives in %.3f ms = %.1f M nodes/s' % (model.n_prim, ms, n / ms / 1e3))


def test_expansion_free_space_frontier_of_the_bench(ctx):
    """The frontier bench.py's `expand` key times (batch.prius_frontier(free_space=True), 2^20 nodes sampled from free
    space + the golden Prius expansion logs embedded): every embedded golden node against the reference's flags and successors, a
    4096-node sample against the oracle, permutation equivariance, and bulk kernel == per-lane kernel on slices (round 3
    checked the uniform frontier only)."""
    from mpc_for_av_at_intersection_amd.batch import prius_frontier
    from oracle import oracle_py as orc
    ex = H.gold('expand.npz')
    gold_nodes = ex['pri/nodes']
    n = 1 << 20
    model, dev = prius_frontier(ctx, n=n, seed=0, free_space=True, embed=gold_nodes)
    nodes = dev.cpu().numpy()
    tables = H.search_tables('prius', 'int_2_1')
    om = orc.SearchModel(*tables)
    out = ctx.expand(model, dev)
    ctx.synchronize()
    col, nbr, cost = out['collide'].cpu().numpy(), out['nbr'].cpu().numpy(), out['cost'].cpu().numpy()
    assert np.array_equal(col[:len(gold_nodes)], ex['pri/collide'])             # the reference's flags on its own nodes
    assert np.abs(nbr[:len(gold_nodes)] - ex['pri/nbr']).max() < 1e-12
    rng = np.random.default_rng(1)
    idx = rng.choice(n, 4096, replace=False)
    onbr, ocol = orc.expand(om, nodes[idx], host_trig=False)
    assert np.array_equal(ocol, col[idx]) and np.abs(onbr - nbr[idx]).max() < 1e-12
    free = 1.0 - col[len(gold_nodes):].mean()
    assert 0.7 < free < 0.95, free                                               # free-space poses: most records survive (uniform frontier: 40 %)
    perm = rng.permutation(n)
    out_p = ctx.expand(model, dev[torch.as_tensor(perm, device=dev.device)].contiguous())
    assert np.array_equal(col[perm], out_p['collide'].cpu().numpy()) and np.array_equal(nbr[perm], out_p['nbr'].cpu().numpy())
    for lo in list(range(0, 120000, 6000)) + [n - 4000]:
        part = ctx.expand(model, dev[lo:lo + 4000].contiguous())
        assert np.array_equal(part['collide'].cpu().numpy(), col[lo:lo + 4000]) and np.array_equal(part['nbr'].cpu().numpy(), nbr[lo:lo + 4000])
        assert np.array_equal(part['cost'].cpu().numpy(), cost[lo:lo + 4000])
    print('free-space frontier: %.1f %% of the records free; golden nodes, oracle sample, permutation and slices identical' % (100 * free))


def test_config2_256_independent_instances_closed_loop(ctx):
    """BASELINE configs[1] on the workload SURVEY 8(d) config 2 defines (batch.config2_batch: route uniform over the 12 stock paths,
    arc position uniform, lateral offset N(0, 0.3 m), heading error N(0, 0.05 rad), v ~ U[0, 8.33], seed 0): batch = 256 independent
    single-ego instances, N = 20, float64 -- the 3 burn-in steps and 12 more, EVERY agent of EVERY step replayed on the oracle from the
    device state of the previous step (decisions and statuses identical, solutions within one 2e-7), the plant update included."""
    from mpc_for_av_at_intersection_amd.batch import ALL_STOCK_PAIRS, config2_batch, stock_routes
    from oracle import oracle_py as orc
    routes, dl, cd = stock_routes(ctx, ALL_STOCK_PAIRS)
    B, T = 256, 20
    sim = config2_batch(ctx, B=B, T=T, seed=0, routes=routes, dl=dl, cd=cd, burn_in=0)
    # the generator itself: perturbed poses (not on the path), speeds over the whole range, all 12 routes drawn
    st0 = sim.state.cpu().numpy()
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy()
    on_path = tab[off + sim.traj_idx.cpu().numpy()]
    lat = np.hypot(st0[:, 0] - on_path[:, 0], st0[:, 1] - on_path[:, 1])
    assert 0.15 < lat.mean() < 0.35 and 0.02 < np.abs(st0[:, 3] - on_path[:, 2]).mean() < 0.06
    assert st0[:, 2].min() < 0.5 and st0[:, 2].max() > 7.8 and len(np.unique(off)) == 12
    po = orc.MpcParams(T=T, L=sim.params.L)
    worst, constrained, n = 0.0, 0, 0
    before = sim.snapshot()
    for step in range(15):
        sim.step()
        after = sim.snapshot()
        assert (after['status'] == 0).all()
        w, it_diff, failed = H.replay_all_on_oracle(sim, before, after, threads=8)
        assert it_diff == 0 and failed == 0
        worst = max(worst, w)
        for q in range(0, B, 8):                         # plant: the oracle's Euler step from the same control reproduces the device state
            nxt = orc.plant_step(po, before['state'][q], after['u'][q, 0, 0], after['u'][q, 1, 0])
            assert np.abs(nxt - after['state'][q]).max() < 1e-9
        if step >= 3:
            constrained += int((after['iters'] > 0).sum()); n += B
        before = after
    print('config 2: 15 steps x 256 agents vs oracle: worst %.2e; %.0f %% of the QPs after burn-in have active constraints' % (worst, 100.0 * constrained / n))
    assert constrained > 0.2 * n                         # "realistic active sets": not a batch of unconstrained minimisers
    sim.check()


def test_closed_loop_run_equals_staged_path_and_graph_replay(ctx):
    """mpcx_closed_loop_run (direct and as a replayed hipGraph on a side stream) against the same kernels driven stage
    by stage through the per-stage entry points: every buffer bit-identical after 6 steps."""
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    routes, dl, cd = stock_routes(ctx)
    sims = {}
    side = Context(0, stream=torch.cuda.Stream(device=0))
    for name, c in (('staged', ctx), ('fused', ctx), ('graph', side)):
        sims[name] = synthetic_batch(c, B=24, A=8, T=13, seed=3, routes=routes, dl=dl, cd=cd)
    torch.cuda.synchronize()
    for _ in range(6):
        sims['staged'].step_staged()
    sims['fused'].run(6)
    sims['graph'].run(2, graph=True)
    sims['graph'].run(4, graph=True)          # second call replays the cached executable graph
    snaps = {k: s.snapshot() for k, s in sims.items()}
    torch.cuda.synchronize()
    assert (snaps['staged']['status'] == 0).all() and snaps['staged']['state'][:, 2].max() > 1.0
    for name in ('fused', 'graph'):
        for key, ref in snaps['staged'].items():
            assert np.array_equal(ref, snaps[name][key]), (name, key)
    # a graph on the null stream is refused loudly, not silently run some other way
    from mpc_for_av_at_intersection_amd.runtime import MpcxError
    with pytest.raises(MpcxError):
        sims['fused'].run(1, graph=True)
    ms, n = ctx.profile_qp_read()
    assert n == 0
    ctx.profile_qp(True)
    sims['fused'].run(3)
    ms, n = ctx.profile_qp_read()
    ctx.profile_qp(False)
    assert n == 3 and ms > 0.0
    side.close()


def test_sensitivity_sweep_as_one_batch(ctx):
    """Per-instance tuning rows (mpcx_set_instance_tuning): 32 closed loops with 32 different weight / limit sets -- the
    sweep of scenarios/mpc_sensitivity_analysis.py -- advanced together; every step of every instance replayed on the
    oracle with that instance's parameters.  Rows equal to the global parameters must change nothing, bit for bit."""
    from dataclasses import replace
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch, stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import MpcParams, MpcxError
    from oracle import oracle_py as orc
    routes, dl, cd = stock_routes(ctx)
    B, T = 32, 13
    rng = np.random.default_rng(5)
    base = MpcParams(T=T, L=cd.distance_back_to_front_wheel)
    sets = []
    for b in range(B):
        sets.append(replace(base, w_perp=float(rng.choice([1.0, 5.0, 20.0, 60.0])), w_para=float(rng.choice([0.2, 1.0, 4.0])),
                            R=(float(rng.choice([0.01, 0.1])), float(rng.choice([0.01, 0.5]))),
                            Rd=(float(rng.choice([0.01, 0.3])), float(rng.choice([0.2, 1.0, 3.0]))),
                            Q_v_yaw=(float(rng.choice([0.0, 1.0])), float(rng.choice([0.1, 0.5, 2.0]))),
                            Qf_base=(1.0, float(rng.choice([1.0, 2.0])), 0.0, float(rng.choice([0.5, 1.0]))),
                            max_accel=float(rng.choice([1.0, 2.0, 3.0])), max_decel=float(rng.choice([-10.0, -5.0])),
                            max_dsteer=float(np.deg2rad(rng.choice([15.0, 30.0, 60.0])))))
    rows = np.stack([s.tuning_row() for s in sets])
    ref = synthetic_batch(ctx, B=B, A=1, T=T, seed=2, routes=routes, dl=dl, cd=cd)
    sim = IntersectionBatch(ctx, base, ref.ip, routes, dl, np.zeros((B, 1), np.int64) + np.arange(B)[:, None] % len(routes),
                            ref.traj_idx.cpu().numpy().reshape(B, 1), tuning=rows)
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    worst = 0.0
    before = sim.snapshot()
    spread = []
    for step in range(8):
        sim.step()
        after = sim.snapshot()
        assert (after['status'] == 0).all()
        for q in range(B):
            po = orc.MpcParams(**{k: getattr(sets[q], k) for k in ('T', 'dt', 'L', 'w_perp', 'w_para', 'R', 'Rd', 'Q_v_yaw', 'Qf_base',
                                                                    'max_accel', 'max_decel', 'max_dsteer')})
            r = orc.agent_step(po, tab[off[q]:off[q] + ln[q]], sim.dl, before['state'][q], np.zeros((0, 6)), int(before['traj_idx'][q]),
                               int(before['prev_cut'][q]), int(before['target_ind'][q]), before['u'][q] if step else None,
                               centers, sim.ip.radius, sim.ip.cutoff_margin)
            assert r['sol'].status == 0 and r['target_ind'] == after['target_ind'][q]
            worst = max(worst, np.abs(r['sol'].u - after['u'][q]).max(), np.abs(r['sol'].x - after['x'][q]).max())
        spread.append(after['u'][:, 0, 0].copy())
        before = after
    assert worst < 2e-7, worst
    assert np.ptp(spread[0]) > 0.5                      # the parameter sets really act (different first accelerations)
    # uniform rows == global parameters: bit-identical to running without rows
    a = synthetic_batch(ctx, B=8, A=8, T=T, seed=4, routes=routes, dl=dl, cd=cd)
    b = synthetic_batch(ctx, B=8, A=8, T=T, seed=4, routes=routes, dl=dl, cd=cd)
    b.tuning = ctx.f64(np.tile(a.params.tuning_row(), (b.P, 1)))
    a.run(5); b.run(5)
    sa, sb = a.snapshot(), b.snapshot()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    # a row count that does not match the batch is an error, not a silent broadcast
    b.tuning = ctx.f64(np.tile(a.params.tuning_row(), (3, 1)))
    with pytest.raises(MpcxError):
        b.run(1)
    ctx.set_instance_tuning(None)
