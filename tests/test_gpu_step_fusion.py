"""GPU tests of step fusion (mpcx_set_step_fusion): mpcx_closed_loop_run takes the plant update of the step before, the pack and prediction
of every agent's pool row and its warm-start rollout in ONE launch (head_kernel) where the run has none of the optional stages.  The launch
evaluates the expressions of plant_kernel, predict_kernel and rollout_kernel, so every buffer must hold the SAME BITS as with the switch
off and as after the per-stage entry points -- compared here with a bitwise test, NaNs included.  The QP work queue is not compared: an
agent's slot inside a key is drawn by an atomic of the conflict search (tests/frontend_helpers.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BURN_IN = 3


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.set_step_fusion(True)
    c.set_instance_tuning(None)
    c.close()


@pytest.fixture(scope='module')
def stock(ctx):
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    return stock_routes(ctx)


def _batch(ctx, stock, B, T=20, seed=11, **kw):
    """B instances x 8 agents on the stock routes after the burn-in (driven without fusion: the parent's launches); the run statistics
    are reset"""
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    routes, dl, cd = stock
    tuning = kw.pop('tuning', None)
    sim = synthetic_batch(ctx, B=B, A=8, T=T, seed=seed, routes=routes, dl=dl, cd=cd, **kw)
    if tuning is not None:
        sim.tuning = ctx.f64(tuning(sim))
    ctx.set_step_fusion(False)
    sim.run(BURN_IN)
    ctx.closed_loop_stats(reset=True)
    return sim


def _arrays(sim):
    """everything a step leaves behind but the work queue (device tensors, the batch's own)"""
    out = dict(state=sim.state, applied=sim.applied, traj_idx=sim.traj_idx, target_ind=sim.target_ind, obs6=sim.obs6,
               u_sol=sim.sol['u'], x_sol=sim.sol['x'], status=sim.sol['status'], iters=sim.sol['iters'], kkt=sim.sol['kkt'],
               xref=sim.pre['xref'], xbar=sim.pre['xbar'], reaches_end=sim.pre['reaches_end'])
    out.update({'inter_' + k: v for k, v in sim.inter.items()})
    if sim.prev_len is not None:
        out['prev_len'] = sim.prev_len
    return out


def _assert_same(a, b, what, stats=None):
    """bit for bit (torch.equal on the bytes: a NaN equals itself)"""
    a.ctx.synchronize(); b.ctx.synchronize()
    xa, xb = _arrays(a), _arrays(b)
    assert sorted(xa) == sorted(xb)
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and xa[k].shape == xb[k].shape, (what, k)
        assert torch.equal(xa[k].contiguous().view(torch.uint8), xb[k].contiguous().view(torch.uint8)), (what, k)
    if stats is not None:
        assert stats[0] == stats[1], (what, stats)


def _drive(ctx, sim, fused, chunks, graph=False):
    """the chunks as one run() each; returns the run statistics of these steps"""
    ctx.set_step_fusion(fused)
    for n in chunks:
        sim.run(n, graph=graph)
    return ctx.closed_loop_stats(reset=True)


# ---- 1. against the per-stage entry points

@pytest.mark.parametrize('B,T', [(1, 20), (9, 20), (9, 13), (2, 32)])
def test_fused_run_equals_host_staging(ctx, stock, B, T):
    """P = 8 (one partial workgroup of the head launch) and P = 72 (a full 64-agent workgroup and a partial one) at T = 20, T = 13 (no
    multiple of the rollout group of 4) and T = 32 at P = 16 (the largest staging buffer, 68 KB): run(6) fused = six step_staged() =
    run(6) without fusion, whose run statistics the fused run must leave too (step_staged() feeds none)"""
    fused, staged, split = (_batch(ctx, stock, B, T) for _ in range(3))
    s_f = _drive(ctx, fused, True, [6])
    for _ in range(6):
        staged.step_staged()
    s_s = _drive(ctx, split, False, [6])
    assert s_f['agent_steps'] == 6 * 8 * B
    _assert_same(fused, staged, 'fused vs staged')
    _assert_same(fused, split, 'fused vs split', (s_f, s_s))


# ---- 2. against the switch, and chunking

def test_chunks_and_the_switch(ctx, stock):
    """seven steps as run(7) fused = run(7) split = run(3) + run(4) fused = 7 x run(1) fused (every call starts with the launch without the
    plant update and ends with plant_kernel)"""
    sims = [_batch(ctx, stock, 9) for _ in range(4)]
    stats = [_drive(ctx, sims[0], True, [7]), _drive(ctx, sims[1], False, [7]), _drive(ctx, sims[2], True, [3, 4]),
             _drive(ctx, sims[3], True, [1] * 7)]
    assert stats[0]['agent_steps'] == 7 * 72 and stats[0]['iterations'] > 0
    for k in (1, 2, 3):
        _assert_same(sims[0], sims[k], 'variant %d' % k, (stats[0], stats[k]))


# ---- 3. failed solves

def _run_with_failures(ctx, stock, **kw):
    """P = 72 with max_iter = 2: the split run step by step (its statuses over the steps must hold failures AND successes), the fused run
    in one call"""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    kw.setdefault('mpc', MpcParams(T=20, max_iter=2))
    split, fused = (_batch(ctx, stock, 9, **kw) for _ in range(2))
    ctx.set_step_fusion(False)
    bad = ok = 0
    for _ in range(6):
        split.run(1)
        ctx.synchronize()
        st = split.sol['status'].cpu().numpy()
        bad += int((st != 0).sum()); ok += int((st == 0).sum())
    s_s = ctx.closed_loop_stats(reset=True)
    print('max_iter = 2, P = 72, 6 steps: %d failed and %d optimal solves' % (bad, ok))
    assert bad > 0 and ok > 0, (bad, ok)
    s_f = _drive(ctx, fused, True, [6])
    assert s_f['failures'] == bad
    _assert_same(fused, split, 'failed solves', (s_f, s_s))


def test_failed_solves(ctx, stock):
    """the plant's fallback (MAX_DECEL, the steering angle kept) and the zeroed warm start that the same launch's rollout must take"""
    _run_with_failures(ctx, stock)


# ---- 4. variants

def test_speed_mode(ctx, stock):
    split, fused = (_batch(ctx, stock, 9, stop_mode='speed') for _ in range(2))
    s_s, s_f = _drive(ctx, split, False, [6]), _drive(ctx, fused, True, [6])
    _assert_same(fused, split, 'speed mode', (s_f, s_s))


def test_instance_tuning_with_failed_solves(ctx, stock):
    """per-instance tuning rows that differ in max_decel (-10 / -5 / -3 by agent), which the failed solves of max_iter = 2 apply"""
    from dataclasses import replace

    def rows(sim):
        return np.stack([replace(sim.params, max_decel=(-10.0, -5.0, -3.0)[q % 3]).tuning_row() for q in range(sim.P)])
    try:
        _run_with_failures(ctx, stock, tuning=rows)
    finally:
        ctx.set_instance_tuning(None)


def test_five_state_model(ctx, stock):
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    split, fused = (_batch(ctx, stock, 9, mpc=MpcParams.jerk()) for _ in range(2))
    s_s, s_f = _drive(ctx, split, False, [6]), _drive(ctx, fused, True, [6])
    _assert_same(fused, split, 'five-state model', (s_f, s_s))


# ---- 5. a host edit between two runs

def test_host_edit_between_runs(ctx, stock):
    """run(2), one agent's state and applied inputs changed from the host, run(2): the head launch reads both at the start of every run"""
    sims = [_batch(ctx, stock, 9) for _ in range(2)]
    stats = []
    for sim, on in zip(sims, (True, False)):
        ctx.set_step_fusion(on)
        sim.run(2)
        ctx.synchronize()
        sim.state[5] += torch.tensor([0.25, -0.1, 0.5, 0.02], dtype=torch.float64, device=sim.state.device)
        sim.applied[5] = torch.tensor([0.05, -1.0], dtype=torch.float64, device=sim.state.device)
        torch.cuda.synchronize()
        sim.run(2)
        stats.append(ctx.closed_loop_stats(reset=True))
    _assert_same(sims[0], sims[1], 'host edit', tuple(stats))


# ---- 6. the runs that keep the launches they had

def test_fallbacks_ignore_the_switch(ctx, stock):
    """a batch with the run log, and a replayed graph, give the same results whatever the switch says"""
    logged = [_batch(ctx, stock, 2) for _ in range(2)]
    logs = [s.attach_log(4) for s in logged]
    stats = [_drive(ctx, logged[0], True, [4]), _drive(ctx, logged[1], False, [4])]
    _assert_same(logged[0], logged[1], 'run log', tuple(stats))
    r0, r1 = logs[0].rows(), logs[1].rows()
    assert r0.dtype == r1.dtype and r0.tobytes() == r1.tobytes()
    from mpc_for_av_at_intersection_amd.runtime import Context
    side = Context(0, stream=torch.cuda.Stream(device=0))       # (a replayed graph needs a stream of its own)
    try:
        graphs = [_batch(side, stock, 2) for _ in range(2)]
        torch.cuda.synchronize()
        stats = [_drive(side, graphs[0], True, [4], graph=True), _drive(side, graphs[1], False, [4], graph=True)]
        _assert_same(graphs[0], graphs[1], 'graph', tuple(stats))
        plain = _batch(ctx, stock, 2)
        s_p = _drive(ctx, plain, True, [4])
        _assert_same(graphs[0], plain, 'graph vs fused', (stats[0], s_p))
    finally:
        side.close()
