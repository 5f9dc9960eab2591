"""The whole MPC step at every horizon the C ABI accepts (mpcx_set_mpc_params: T = 1 .. MPCX_T_MAX = 32), not only at the stock
T = 10 / 13 / 20: the reference window and rollout against the reference's own output (mpc_pre_horizons.npz), both QP solvers against
the oracle and the exact minimiser at every T, per-instance tuning and the five-state controller at long horizons, and the batched
closed loop replayed agent by agent on the oracle.  What changes with T: the stage solver's stages per lane (SPL = 2 for T <= 16, 3 for
T <= 24, 4 above), the condensed solver's buckets (qp_kernel<10 / 13 / 20 / 32>), the window's lane T (lane 32 at T = 32), the
rollout's staging buffer (above 64 KB of dynamic LDS for T >= 31), the plant's and the loop's strides (2T, T + 1)."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

BAR = 5e-6          # |z_gpu - z_exact| (tests/test_gpu_accuracy.py)
QP_TOL = 2e-7       # |GPU - oracle| of the five-state controller and of a replayed closed loop (tests/test_gpu_jerk.py, test_gpu_fullsize.py)


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    from mpc_for_av_at_intersection_amd.lib import _session
    c = Context(0)
    yield c
    if _session._ctx is c:          # synthetic_batch() made this context the drop-in classes' session context: do not leave a closed one behind
        _session.set_context(None)
    c.close()


@pytest.mark.parametrize('T', H.HORIZON_FIXTURE_TS)
def test_prepare_at_every_fixture_horizon(ctx, T):
    """mpcx_mpc_prepare_batch on the reference's window / rollout cases at T, tiled to B = 1000 (16 rollout workgroups, the last one
    partly filled): target index, window and reaches_end bit-exact, rollout <= 1e-12 (test_gpu_parity.py::test_prepare_vs_golden).
    T = 31 / 32: the rollout's staging buffer is 66 / 68 KB of dynamic LDS.  (The forked rollout of the closed loop is checked by
    test_closed_loop_every_agent_on_the_oracle.)"""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    g = H.gold('mpc_pre_horizons.npz')
    k = 'T%d/' % T
    n = len(g[k + 'state'])
    idx = np.arange(1000) % n
    ctx.set_mpc_params(MpcParams(T=T))
    routes = sorted({(int(sp), int(ti)) for sp, ti, _ in g[k + 'path']})
    full = {r: H.smoothed_path(*r) for r in routes}
    base = dict(zip(routes, np.cumsum([0] + [len(full[r]) for r in routes])[:-1]))
    path = np.concatenate([full[r] for r in routes])
    off = np.array([base[(sp, ti)] for sp, ti, _ in g[k + 'path']])[idx]
    ln = g[k + 'path'][idx, 2]
    dl = float(np.linalg.norm(path[0, :2] - path[1, :2]))
    uw = np.stack([g[k + 'oa'], g[k + 'od']], axis=1)[idx]
    tind = ctx.i32(g[k + 'start'][idx])
    out = ctx.prepare(ctx.f64(g[k + 'state'][idx]), ctx.f64(uw), ctx.f64(path), ctx.i32(off), ctx.i32(ln), dl, tind)
    ctx.synchronize()
    assert np.array_equal(tind.cpu().numpy(), g[k + 'target_ind'][idx])
    assert np.array_equal(out['reaches_end'].cpu().numpy(), g[k + 'reaches_end'][idx])
    assert np.array_equal(out['xref'].cpu().numpy(), g[k + 'xref'][idx])
    d = np.abs(out['xbar'].cpu().numpy() - g[k + 'xbar'][idx]).max()
    assert d < 1e-12, d


_HARVEST = {}


def _problems(ctx, T):
    """the oracle-built problems of helpers.horizon_problems at T, plus at T in {16, 24, 25, 32} problems harvested from the batched
    closed loop at T (every one that took >= 8 iterations there, topped up with a sample)"""
    probs = H.stack_problems(H.horizon_problems(T, n=24))
    if T in (16, 24, 25, 32):
        if T not in _HARVEST:
            c = H.harvest_closed_loop_qps(ctx, B=96, A=8, T=T, total=160, hard_iters=8, windows=((2, 2), (30, 2)))
            _HARVEST[T] = [c['x0'], c['xref'], c['xbar'], c['re'].astype(np.uint8), c['uw']]
        probs = [np.concatenate([a, b]) for a, b in zip(probs, _HARVEST[T])]
    return probs


def _solve(ctx, which, probs):
    ctx.set_qp_solver(which)
    try:
        out = ctx.qp_solve(*(ctx.u8(a) if i == 3 else ctx.f64(a) for i, a in enumerate(probs)))
        ctx.synchronize()
    finally:
        ctx.set_qp_solver('auto')
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('T', range(1, 33))
def test_both_solvers_at_every_horizon(ctx, T):
    """stage-structured and condensed solver, forced, at T against the oracle: same status, same iteration count on >= 98 % of the
    problems and within one elsewhere (test_gpu_parity.py::test_qp_stage_solver_equals_condensed_solver).  Solutions: x within 1e-9 of
    the oracle for the stage solver, u within 1e-8 -- the bar of the host build of the same solver header against the same oracle
    (tests/test_stage_ref.py): on these warm-started, mostly constrained problems the Riccati recursion and the oracle's dense solve
    round apart by up to 2.1e-9 in u (T = 17), identically in the one-lane host build and on the GPU, while both sit 1e-8 .. 2e-7 from
    the exact minimiser; an indexing error moves u by O(1).  Condensed solver: u within 1e-8 and x within 1e-8 up to T = 20, 5e-6 /
    5e-5 above (its 64 x 64 condensed system is the less accurate of the two there -- the bar test_qp_stage_solver_equals_condensed_solver
    keeps at T = 32).  At horizons of each stage-solver width (SPL 2 / 3 / 4: T = 9, 11, 16 / 17, 24 / 25, 32) and each condensed bucket
    (qp_kernel<10 / 13 / 20 / 32>: T = 9, 11, 16 / 17, 24 / 25 / 32) both also against the exact minimiser (tests/qp_literal.py)."""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    from oracle import oracle_py as orc
    from tests import qp_literal as QL
    x0, xref, xbar, re, uw = probs = _problems(ctx, T)
    n = len(x0)
    po = orc.MpcParams(T=T)
    ref = [orc.qp_solve(po, x0[k], xref[k], xbar[k], re[k], uw[k]) for k in range(n)]
    r_status = np.array([r.status for r in ref]); r_iters = np.array([r.iters for r in ref])
    ctx.set_mpc_params(MpcParams(T=T))
    res = {w: _solve(ctx, w, probs) for w in ('stage', 'condensed')}
    ok = r_status == 0
    assert ok.mean() > 0.9
    for w, o in res.items():
        assert np.array_equal(o['status'], r_status), (w, o['status'], r_status)
        it = o['iters'].astype(int)
        assert np.abs(it[ok] - r_iters[ok]).max() <= 1 and (it[ok] == r_iters[ok]).mean() >= 0.98, (w, it, r_iters)
        du = max(np.abs(o['u'][k] - ref[k].u).max() for k in np.nonzero(ok)[0])
        dx = max(np.abs(o['x'][k] - ref[k].x).max() for k in np.nonzero(ok)[0])
        tol_u, tol_x = (1e-8, 1e-9) if w == 'stage' else (1e-8, 1e-8) if T <= 20 else (5e-6, 5e-5)
        print('T=%2d %-9s %3d problems (%3d constrained): |du| %.2e |dx| %.2e' % (T, w, n, int((r_iters > 0).sum()), du, dx))
        assert du < tol_u and dx < tol_x, (w, du, dx)
    if T in (16, 24, 32):           # the problems are not all easy: a real share has active constraints
        assert (r_iters > 0).mean() >= 0.3, (r_iters > 0).mean()
    if T in (9, 11, 16, 17, 24, 25, 32):
        sel = np.nonzero(ok)[0]
        sel = np.concatenate([sel[r_iters[sel] > 0][:10], sel[r_iters[sel] == 0][:2]])
        worst = {}
        for k in sel:
            ex = None
            for w, o in res.items():
                z = QL.pack(po, o['x'][k], o['u'][k])
                if ex is None:
                    ex = QL.exact_solution(po, x0[k], xref[k], xbar[k], re[k], z)
                    assert ex['eq'] < 1e-9 and (ex['lam'] >= -1e-7).all() and ex['slack'].min() > -1e-9, k
                worst[w] = max(worst.get(w, 0.0), float(np.abs(z - ex['z']).max()))
        print('T=%2d vs the exact minimiser (%d problems): %s' % (T, len(sel), worst))
        assert max(worst.values()) < BAR, worst


@pytest.mark.parametrize('T', [24, 32])
def test_instance_tuning_at_long_horizons(ctx, T):
    """per-instance tuning rows (mpcx_set_instance_tuning) at T = 24 / 32 -- qp_quad_kernel<8, 3, true> / <8, 4, true> -- in the
    closed loop: every step of every instance against the oracle with that instance's own parameters
    (tests/test_gpu_fullsize.py::test_sensitivity_sweep_as_one_batch, there at T = 13)"""
    from dataclasses import replace
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch, stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    from oracle import oracle_py as orc
    routes, dl, cd = stock_routes(ctx)
    B = 21
    rng = np.random.default_rng(T)
    base = MpcParams(T=T, L=cd.distance_back_to_front_wheel)
    sets = [replace(base, w_perp=float(rng.choice([1.0, 5.0, 20.0, 60.0])), w_para=float(rng.choice([0.2, 1.0, 4.0])),
                    R=(float(rng.choice([0.01, 0.1])), float(rng.choice([0.01, 0.5]))),
                    Rd=(float(rng.choice([0.01, 0.3])), float(rng.choice([0.2, 1.0, 3.0]))),
                    Q_v_yaw=(float(rng.choice([0.0, 1.0])), float(rng.choice([0.1, 0.5, 2.0]))),
                    Qf_base=(1.0, float(rng.choice([1.0, 2.0])), 0.0, float(rng.choice([0.5, 1.0]))),
                    max_accel=float(rng.choice([1.0, 2.0, 3.0])), max_decel=float(rng.choice([-10.0, -5.0])),
                    max_dsteer=float(np.deg2rad(rng.choice([15.0, 30.0, 60.0])))) for _ in range(B)]
    rows = np.stack([s.tuning_row() for s in sets])
    ref = synthetic_batch(ctx, B=B, A=1, T=T, seed=2, routes=routes, dl=dl, cd=cd)
    sim = IntersectionBatch(ctx, base, ref.ip, routes, dl, np.zeros((B, 1), np.int64) + np.arange(B)[:, None] % len(routes),
                            ref.traj_idx.cpu().numpy().reshape(B, 1), tuning=rows)
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    worst, n_con, spread = 0.0, 0, []
    before = sim.snapshot()
    ctx.set_qp_solver('stage')
    try:
        for step in range(5):
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
                n_con += int(r['sol'].iters > 0)
            spread.append(after['u'][:, 0, 0].copy())
            before = after
    finally:
        ctx.set_qp_solver('auto')
        ctx.set_instance_tuning(None)
    print('T=%d tuned: worst |GPU - oracle| %.2e, %d of %d solves constrained' % (T, worst, n_con, 5 * B))
    assert worst < QP_TOL, worst
    assert np.ptp(spread[0]) > 0.5 and n_con > 0


@pytest.mark.parametrize('T', [16, 17, 24, 25, 32])
def test_jerk_controller_at_long_horizons(ctx, T):
    """the five-state controller (MpcParams.jerk(T)) on real windows made at T (helpers.horizon_problems, not padded ones): statuses
    identical to the jerk oracle, solutions within QP_TOL, iteration counts as tests/test_gpu_jerk.py allows, and against the exact
    minimiser of the literal five-state problem (max < 5e-6, median < 1e-7)"""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    from oracle import oracle_py as orc
    from tests import qp_literal as QL
    x0, xref, xbar, re, uw = H.stack_problems(H.horizon_problems(T, n=16))
    n = len(x0)
    ctx.set_mpc_params(MpcParams.jerk(T=T))
    out = ctx.qp_solve(ctx.f64(x0), ctx.f64(xref), ctx.f64(xbar), ctx.u8(re), ctx.f64(uw))
    ctx.synchronize()
    u, x = out['u'].cpu().numpy(), out['x'].cpu().numpy()
    status, iters = out['status'].cpu().numpy(), out['iters'].cpu().numpy()
    po = orc.MpcParams.jerk(T=T)
    worst, dist, it_diff, n_con = 0.0, [], 0, 0
    for k in range(n):
        sol = orc.qp_solve(po, x0[k], xref[k], xbar[k], re[k], uw[k])
        assert sol.status == status[k] == 0, (k, sol.status, status[k])
        worst = max(worst, np.abs(sol.u - u[k]).max(), np.abs(sol.x[:4] - x[k]).max())
        it_diff += int(sol.iters != iters[k])
        n_con += int(sol.iters > 0)
        x4 = (x[k, 2, 1] - x[k, 2, 0]) / po.dt - u[k, 0, 0] + po.dt * np.concatenate([[0.0], np.cumsum(u[k, 0])])
        z = QL.pack(po, np.vstack([x[k], x4]), u[k])
        ex = QL.exact_solution(po, x0[k], xref[k], xbar[k], re[k], z)
        dist.append(np.abs(z - ex['z']).max())
    dist = np.array(dist)
    print('T=%d jerk: %d problems (%d constrained): |gpu - oracle| %.2e, |gpu - exact| max %.2e median %.2e, %d iteration counts differ'
          % (T, n, n_con, worst, dist.max(), np.median(dist), it_diff))
    assert worst < QP_TOL and it_diff <= max(1, n // 20)
    assert dist.max() < 5e-6 and np.median(dist) < 1e-7
    assert n_con >= n // 4


def _check_windows(sim, before, after):
    """the step's reference window (bit-exact) and rollout (<= 1e-12) of every agent, made in the closed loop with the rollout forked
    beside the conflict search, against the oracle's from the state before the step (one linearisation pass)"""
    from oracle import oracle_py as orc
    import dataclasses
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy()
    worst, n = 0.0, 0
    for q in np.nonzero(after['target_ind'] >= 0)[0]:
        path = tab[off[q]:off[q] + after['cut_len'][q]]
        xref, s, re = orc.calc_ref_trajectory(po, before['state'][q], path[:, 0], path[:, 1], path[:, 2], sim.dl, int(before['target_ind'][q]))
        assert s == after['target_ind'][q] and np.array_equal(xref, after['xref'][q]) and np.array_equal(re, after['reaches_end'][q]), q
        xbar = orc.predict_motion(po, before['state'][q], before['u'][q, 0], before['u'][q, 1])
        worst = max(worst, float(np.abs(xbar - after['xbar'][q]).max()))
        n += 1
    assert n > 0.9 * len(after['target_ind']) and worst < 1e-12, (n, worst)


@pytest.mark.parametrize('T,solver', [(1, 'auto'), (1, 'stage'), (16, 'auto'), (16, 'stage'), (24, 'auto'), (24, 'stage'),
                                      (25, 'auto'), (31, 'auto'), (32, 'auto')])
def test_closed_loop_every_agent_on_the_oracle(ctx, T, solver):
    """the batched closed loop (mpcx_closed_loop_run: rollout forked beside the conflict search, window, solve, plant) at T on the
    stock routes, 13 instances x 7 agents (91 agents: two rollout workgroups, the second partly filled): after a few steps, EVERY
    agent of two steps replayed on the oracle (helpers.replay_all_on_oracle, 2e-7), and the window / rollout of every agent checked.
    'auto' picks the condensed solver at T <= 20 for a batch this small and the stage solver above; 'stage' forces the latter."""
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    routes, dl, cd = stock_routes(ctx)
    sim = synthetic_batch(ctx, B=13, A=7, T=T, seed=T, routes=routes, dl=dl, cd=cd)
    ctx.set_qp_solver(solver)
    try:
        sim.run(3)
        before = sim.snapshot()
        worst, n_con = 0.0, 0
        for _ in range(2):
            sim.step()
            after = sim.snapshot()
            w, it_diff, failed = H.replay_all_on_oracle(sim, before, after)
            _check_windows(sim, before, after)
            assert it_diff <= 1 and failed == 0, (it_diff, failed)
            worst = max(worst, w)
            n_con += int((after['iters'] > 0).sum())
            before = after
    finally:
        ctx.set_qp_solver('auto')
    print('T=%d %s closed loop: 2 x %d agents replayed, worst |GPU - oracle| %.2e, %d constrained solves' % (T, solver, sim.P, worst, n_con))
    assert T == 1 or n_con > 0


def test_closed_loop_t32_two_passes_and_one_call_of_n_steps(ctx):
    """T = 32: (1) two linearisation passes -- the second pass's window reads the first pass's speeds at stride T + 1 -- through
    mpcx_closed_loop_run equal, bit for bit, the same passes driven stage by stage (Context.prepare with x_prev), and the second
    pass's window equals the oracle's window spaced by the solution's speeds; (2) one mpcx_closed_loop_run of n steps equals n calls of
    one step bit for bit (tests/test_gpu_edges.py::test_one_call_of_n_steps_equals_n_calls_of_one_step)"""
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    from oracle import oracle_py as orc
    import dataclasses
    T = 32
    sims = [synthetic_batch(ctx, B=13, A=7, T=T, seed=5) for _ in range(3)]
    sims[0].lin_passes = sims[1].lin_passes = 2
    for _ in range(4):
        sims[0].run(1)
        sims[1].step_staged()
        sims[2].run(1)
    a, b, c = (s.snapshot() for s in sims)
    for k in ('state', 'u', 'x', 'target_ind', 'cut_len', 'status', 'xref', 'xbar', 'iters'):
        assert np.array_equal(a[k], b[k]), k
    assert (a['status'] == 0).all() and not np.array_equal(a['u'], c['u'])
    # the window with the previous pass's speeds, against the oracle's (the device's speeds as ov)
    sim = sims[2]
    ctx.set_mpc_params(sim.params)
    tind = sim.target_ind.clone()
    out = ctx.prepare(sim.state, sim.sol['u'], sim.path, sim.path_off, sim.inter['cut_len'], sim.dl, tind, x_prev=sim.sol['x'])
    ctx.synchronize()
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy()
    xr, re, ti = out['xref'].cpu().numpy(), out['reaches_end'].cpu().numpy(), tind.cpu().numpy()
    for q in range(sim.P):
        path = tab[off[q]:off[q] + c['cut_len'][q]]
        xref, s, r = orc.calc_ref_trajectory(po, c['state'][q], path[:, 0], path[:, 1], path[:, 2], sim.dl, int(c['target_ind'][q]), ov=c['x'][q, 2])
        assert s == ti[q] and np.array_equal(xref, xr[q]) and np.array_equal(r, re[q]), q
    # one call of n steps == n calls of one step
    s1, s2 = (synthetic_batch(ctx, B=13, A=7, T=T, seed=9) for _ in range(2))
    ctx.closed_loop_stats(reset=True)
    s1.run(3); s1.run(5)
    st_a = ctx.closed_loop_stats(reset=True)
    for _ in range(8):
        s2.run(1)
    st_b = ctx.closed_loop_stats(reset=True)
    a, b = s1.snapshot(), s2.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert st_a == st_b and st_a['agent_steps'] == 8 * s1.P, (st_a, st_b)
    assert (a['status'] == 0).all()
