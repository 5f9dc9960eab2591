"""Per-problem tuning rows (mpcx_set_instance_tuning) through every QP kernel that reads them, with rows that really differ from problem to
problem and lie away from the stock parameters: qp_quad_kernel<8, 2 / 3 / 4, true, false> and <8, *, true, true> of the stage solver (each
8-lane group of a wavefront replaces weights and limits from its own row, QueueSrc::fetch) and the has_tune path of the condensed
qp_kernel<10 / 13 / 20 / 32>.  Neither bench.py nor smoke() sets a row: this file and the closed-loop sweeps are their only protection.

Inputs: tests/tuning_helpers.mixed -- 24 warm-started problems per horizon, problem i under set i % 16 of the sweep lattice, so that the
eight groups of a wavefront always sit on eight different rows.  The reference side (oracle, one-lane host build, exact minimiser, each
problem under its own set) is pinned on the CPU by tests/test_tuning_cpu.py.

(a) every tuned instantiation against the oracle and the exact minimiser; (b) the same bits whatever the schedule, order hint included
(a.tune[order[t]]); (c) uniform rows == global parameters away from stock; (d) more problems than lane groups / wavefronts, so that a
group draws a second problem with another row; (e) the coupled closed loop with one row per agent replayed on the oracle."""
import numpy as np
import pytest
import torch

from tests import tuning_helpers as TH

pytestmark = pytest.mark.gpu

QP_TOL = 2e-7                   # |GPU - oracle| (tests/test_gpu_horizons.py, test_gpu_fullsize.py)
BAR, BAR_MEDIAN = 5e-6, 1e-7    # |GPU - exact minimiser|, worst problem and median (tests/test_gpu_accuracy.py, test_gpu_horizons.py)


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


CASES_A = [('stage', T, False) for T in (13, 16, 20, 24, 32)] + [('condensed', T, False) for T in (10, 13, 20, 32)] + \
          [('stage', T, True) for T in (13, 20, 28)]


@pytest.mark.parametrize('solver,T,jerk', CASES_A, ids=['%s-%s%d' % (s, 'jerk' if j else 'T', T) for s, T, j in CASES_A])
def test_every_tuned_kernel_against_oracle_and_exact_minimiser(ctx, solver, T, jerk):
    """One launch of the 24 mixed problems with their 24 rows, the global parameters at stock (MpcParams.jerk(T) for the five-state
    model): status identical to the oracle's under each problem's own set, iteration count within one, u and x within 2e-7 (the forced
    condensed solver at T = 32: 5e-6 / 5e-5, its bars in test_both_solvers_at_every_horizon); and within 5e-6 (max) / 1e-7 (median) of the
    exact minimiser of the literal problem under that set (condensed at T = 32: printed only).  A kernel that read another problem's row,
    dropped a field or kept a constant of the group's previous problem moves u by O(0.1).
    Measured on an MI355X (iteration counts identical to the oracle's in all twelve cases), |GPU - oracle| and |GPU - exact| max:
    stage T = 13 / 16 / 20 / 24 / 32: 1.3e-10 / 5.1e-11 / 2.5e-11 / 6.4e-11 / 2.6e-11 and 2.0e-9 / 2.0e-9 / 2.6e-8 / 5.5e-9 / 1.6e-8;
    condensed T = 10 / 13 / 20 / 32: 3.3e-11 / 4.7e-11 / 1.6e-11 / 3.9e-11 and 1.1e-8 / 2.0e-9 / 2.6e-8 / 1.6e-8;
    five-state T = 13 / 20 / 28: 6.9e-11 / 7.5e-10 / 6.0e-10 and 4.5e-10 / 1.4e-8 / 1.5e-8; medians against the exact point 1e-11 .. 2e-10."""
    m, ref = TH.mixed(T, jerk), TH.reference(T, jerk)
    out = TH.solve(ctx, solver, m.base, m.arrays, rows=m.rows)
    assert np.array_equal(out['status'], ref.status), (out['status'], ref.status)
    assert (ref.status == 0).all()
    it = out['iters'].astype(int)
    assert np.abs(it - ref.iters).max() <= 1, (it, ref.iters)
    du = np.array([np.abs(out['u'][k] - ref.sol[k].u).max() for k in range(24)])
    dx = np.array([np.abs(out['x'][k] - ref.sol[k].x[:4]).max() for k in range(24)])
    dist = np.array([np.abs(TH.pack_device(m.oracle[k], out['x'][k], out['u'][k]) - ref.exact[k]['z']).max() for k in range(24)])
    print('%s %s T=%d tuned: |du| %.2e (problem %d) |dx| %.2e (problem %d), |gpu - exact| max %.2e (problem %d) median %.2e, %d iteration counts differ'
          % (solver, 'five-state' if jerk else 'four-state', T, du.max(), du.argmax(), dx.max(), dx.argmax(), dist.max(), dist.argmax(),
             np.median(dist), int((it != ref.iters).sum())))
    loose = solver == 'condensed' and T == 32
    tol_u, tol_x = (5e-6, 5e-5) if loose else (QP_TOL, QP_TOL)
    assert du.max() < tol_u and dx.max() < tol_x, (du, dx)
    if not loose:
        assert dist.max() < BAR and np.median(dist) < BAR_MEDIAN, dist


@pytest.mark.parametrize('solver', ['stage', 'condensed'])
@pytest.mark.parametrize('T', [13, 20])
def test_schedule_independence_with_rows(ctx, solver, T):
    """the same 24 problems and rows as they lie, with problems and rows both reversed, and as they lie under an order hint that reverses
    the queue (hint i for problem i: 24 distinct keys, longest first): x, u, status, iters and kkt bit-identical per problem.  Under the
    hint the ticket t and the problem order[t] differ for every draw: a kernel that read tune[t] would solve with another problem's row."""
    m = TH.mixed(T)
    rev = np.arange(24)[::-1].copy()
    lie = TH.solve(ctx, solver, m.base, m.arrays, rows=m.rows)
    turned = TH.solve(ctx, solver, m.base, TH.take(m.arrays, rev), rows=m.rows[rev])
    hinted = TH.solve(ctx, solver, m.base, m.arrays, rows=m.rows, hint=np.arange(24))
    assert (lie['status'] == 0).all() and (lie['iters'] > 0).sum() >= 20
    TH.assert_same_bits(lie, turned, '%s T=%d, reversed' % (solver, T), ib=rev)
    TH.assert_same_bits(lie, hinted, '%s T=%d, reversing order hint' % (solver, T))


CASES_C = [('stage', 13, False), ('condensed', 13, False), ('stage', 20, False), ('condensed', 20, False), ('stage', 13, True)]


@pytest.mark.parametrize('solver,T,jerk', CASES_C, ids=['%s-%s%d' % (s, 'jerk' if j else 'T', T) for s, T, j in CASES_C])
def test_uniform_rows_equal_global_parameters_away_from_stock(ctx, solver, T, jerk):
    """sets 0, 7 and 14: the 24 problems under set_mpc_params(set) without rows, and under the stock parameters with 24 copies of the set's
    row: all five fields bit-identical (the untuned and the tuned instantiation compute the same thing from the same numbers).
    This test found the stage solver's two instantiations apart by rounding (same status and iteration counts; u up to 3.2e-11, x up to
    4.4e-12, kkt up to 1.0e-9, on 4 to 23 of the 24 problems, at the stock parameters as well): in the cost gradient's sums of two
    products the compiler fused the other product where the weights are per-lane values.  csrc/mpcx_qp_stage.h now spells those fused
    multiply-adds out as the kernels without rows have always had them.  Measured on an MI355X since: bit-identical in all five cases."""
    m = TH.mixed(T, jerk)
    stock = TH.solve(ctx, solver, m.base, m.arrays)
    for s in (0, 7, 14):
        p = TH.runtime_params(T, jerk, **m.sets[s])
        glob = TH.solve(ctx, solver, p, m.arrays)
        rows = TH.solve(ctx, solver, m.base, m.arrays, rows=np.tile(p.tuning_row(), (24, 1)))
        assert (glob['status'] == 0).all() and (glob['iters'] > 0).any()
        assert not np.array_equal(glob['u'], stock['u'])        # the set acts
        print('%s %s T=%d set %d, global parameters vs uniform rows, max difference: %s'
              % (solver, 'five-state' if jerk else 'four-state', T, s, {k: '%.1e' % np.abs(glob[k].astype(float) - rows[k].astype(float)).max() for k in TH.FIELDS}))
        TH.assert_same_bits(glob, rows, '%s T=%d set %d: global parameters vs uniform rows' % (solver, T, s))


@pytest.mark.parametrize('solver,T', [('stage', 13), ('stage', 20), ('condensed', 20)])
def test_second_draw_with_another_row(ctx, solver, T):
    """More problems than the launch has lane groups (stage: min(ceil(B / 8), 4 CUs) wavefronts of eight, B = 32 CUs + 8 * 19) or wavefronts
    (condensed: min(B, 4 CUs), B = 4 CUs + 19), so that some draw a second problem -- with another row, after the refill.  Problem j is
    problem j % 24 under row j % 16: 48 distinct (problem, row) pairs, every output bit-identical to its pair's in one launch of the 48,
    where nobody draws twice.  Twice: in queue order, and under an order hint (keys j % 9), where in addition ticket != problem."""
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    B = 32 * cus + 8 * 19 if solver == 'stage' else 4 * cus + 19
    assert B > (32 if solver == 'stage' else 4) * cus
    m = TH.mixed(T)
    j = np.arange(B)
    pairs = np.arange(48)
    small = TH.solve(ctx, solver, m.base, TH.take(m.arrays, pairs % 24), rows=m.rows[pairs % 16])
    assert (small['status'] == 0).all()
    assert len({small['u'][k].tobytes() for k in range(48)}) == 48                            # the row changes the answer of every problem
    for hint in (None, j % 9):
        big = TH.solve(ctx, solver, m.base, TH.take(m.arrays, j % 24), rows=m.rows[j % 16], hint=hint)
        TH.assert_same_bits(big, small, '%s T=%d, B=%d (%d CUs), %s' % (solver, T, B, cus, 'queue order' if hint is None else 'order hint'), ib=j % 48)


@pytest.mark.parametrize('solver', ['stage', 'auto'])
def test_coupled_closed_loop_with_a_row_per_agent(ctx, solver):
    """IntersectionBatch(tuning=(B * A, 16)): 2 instances x 8 agents at T = 20 on the stock routes (tuning_helpers.loop_scene: the layout of
    synthetic_batch(seed=0)), agent q under set q % 16, six steps; 'auto' takes the condensed solver at this size.  After every step every
    agent replayed with orc.agent_step under its own parameters and with its instance mates' rows as obstacles
    (tests/test_gpu_conflict_wide.py::_replay_egos): traj_idx, cut length, target index, hit index and status identical, u and x within
    2e-7.  On the CPU oracle (tests/test_tuning_cpu.py) 86 of the 96 agent-steps have a conflict and 27 solves are constrained; both are
    asserted here from the replay.  Measured on an MI355X: the same counts, worst |GPU - oracle| 7.9e-12 (stage) / 1.8e-11 (auto)."""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams
    from oracle import oracle_py as orc
    sc = TH.loop_scene()
    L = sc.cd.distance_back_to_front_wheel
    base = TH.runtime_params(sc.T, L=L)
    po = [TH.oracle_params(sc.T, L=L, **s) for s in sc.sets]
    rows = np.stack([TH.runtime_params(sc.T, L=L, **s).tuning_row() for s in sc.sets])
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(sc.cd.radius / sc.dl)), L=L, radius=sc.cd.radius, circle_centers=np.asarray(sc.cd.circle_centers).ravel())
    sim = IntersectionBatch(ctx, base, ip, sc.routes, sc.dl, sc.route_of, sc.start, tuning=rows)
    assert tuple(sim.tuning.shape) == (16, 16)
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    o_off, o_cnt, o_skip = (t.cpu().numpy() for t in (sim.obs_off, sim.obs_cnt, sim.obs_skip))
    centers = np.asarray(sim.ip.circle_centers).reshape(2, 2)
    worst, n_hit, n_con = 0.0, 0, 0
    ctx.set_qp_solver(solver)
    try:
        before = sim.snapshot()
        for step in range(TH.LOOP['steps']):
            sim.step()
            after = sim.snapshot()
            pool = np.column_stack([before['state'], before['applied'][:, 1], before['applied'][:, 0]])
            for p in range(sim.P):
                present = [r for r in range(o_off[p], o_off[p] + o_cnt[p]) if r != o_skip[p]]
                r = orc.agent_step(po[p], tab[off[p]:off[p] + ln[p]], sim.dl, before['state'][p], pool[present], int(before['traj_idx'][p]),
                                   int(before['prev_cut'][p]), int(before['target_ind'][p]), before['u'][p], centers, sim.ip.radius, sim.ip.cutoff_margin)
                want_hit = -1 if r['hit'] is None else int(r['hit'][2])
                got = (after['traj_idx'][p], after['cut_len'][p], after['target_ind'][p], after['hit_idx'][p], after['status'][p])
                assert (r['traj_idx'], r['cut'], r['target_ind'], want_hit, r['sol'].status) == got, (step, p, r['traj_idx'], r['cut'], r['target_ind'], want_hit, got)
                assert r['sol'].status == 0, (step, p)
                worst = max(worst, float(np.abs(r['sol'].u - after['u'][p]).max()), float(np.abs(r['sol'].x - after['x'][p]).max()))
                n_hit += int(want_hit >= 0); n_con += int(r['sol'].iters > 0)
            before = after
    finally:
        ctx.set_qp_solver('auto')
        ctx.set_instance_tuning(None)
    print('%s closed loop with a row per agent: %d agent-steps on the oracle, %d with a conflict, %d constrained, worst |GPU - oracle| %.2e'
          % (solver, TH.LOOP['steps'] * sim.P, n_hit, n_con, worst))
    assert worst < QP_TOL, worst
    assert n_hit > 0 and n_con > 0
