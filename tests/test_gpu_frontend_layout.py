"""GPU tests of the front end's lane layout: rollout_kernel (a group of lanes per instance) and ref_window_kernel (several agents per
wavefront, a run of T + 1 lanes per window).  The layout only moves who computes a value, never the operations or their order, so
(1) seeded closed loops give the bits the parent build gave (tests/golden/frontend_parent.npz, recorded by
scripts/record_frontend_parent.py), (2) the shapes at which the packing can go wrong agree with the oracle's rollout and window functions
at the tolerances of tests/test_gpu_parity.py (indices and xref exact, device-trig coordinates 1e-12), (3) the work queue the window
kernel scatters is a permutation of the filed agents, keys descending."""
import numpy as np
import pytest
import torch

from tests import frontend_helpers as FH
from tests import helpers as H

pytestmark = pytest.mark.gpu
TRIG_TOL = 1e-12        # device libm against the host's sin / cos / tan over at most 64 steps (tests/test_gpu_parity.py's bound)


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


# ---- 1. bit identity with the parent build

@pytest.mark.parametrize('name', FH.SCENARIOS)
def test_same_bits_as_the_parent_build(ctx, stock, name):
    """step 1 after the burn-in and the steps with a fresh cut scan the path (hint miss), the others take the conflict search's answer (hint
    hit); 'scene' has agents retired from the start and arrivals on the way, 'stand' agents that wait outside the scene and enter later.
    The queue is compared as its keys along the order and the agents of every key (FH.run: their places inside a key are drawn by an atomic
    of the conflict search and differ between two runs of the parent build itself); the prediction by its digest."""
    gold = H.gold('frontend_parent.npz')
    assert len(str(gold['parent_commit'])) == 40
    got = FH.run(ctx, stock, name)
    keys = [k for k in gold.files if k.startswith(name + '/')]
    assert sorted(keys) == sorted(got) and len(keys) == len(FH.COMPARED_STEPS) * (len(FH.KEYS) + 1) + 3
    for k in keys:
        assert got[k].dtype == gold[k].dtype and np.array_equal(got[k], gold[k]), k
    if name != 'traffic':      # the fixture covers what it is there for: somebody retired or waiting, and that set changes on the way
        d = [gold['%s/%d/done' % (name, s)] for s in FH.COMPARED_STEPS]
        assert d[0].any() and not np.array_equal(d[0], d[-1])
        assert 0 < len(gold['%s/order' % name]) < FH.B * FH.A


# ---- 2. shapes at which the packing can go wrong

def _paths():
    """three stock paths and, last, a zig-zag whose three nearest points to (2.9, 0.1) are the indices 3, 0, 6: calc_nearest_index_in_direction
    raises 'something wrong' there (target_ind = -1)"""
    paths = [H.smoothed_path(4, 1), H.smoothed_path(1, 2), H.smoothed_path(2, 1)]
    k = np.arange(12.0)
    paths.append(np.column_stack([k, np.where(k % 3 == 0, 0.0, 50.0), np.zeros(12)]))
    return paths


def _window_case(B, T, seed, degenerate=None):
    """B agents spread over the stock paths, off the path by a little, a random warm start; agent `degenerate` sits on the zig-zag"""
    rng = np.random.default_rng(seed)
    paths = _paths()
    offs = np.cumsum([0] + [len(p) for p in paths])
    which = rng.integers(0, 3, B)
    start = np.array([rng.integers(0, len(paths[w]) - 3) for w in which])
    state = np.zeros((B, 4))
    for b in range(B):
        pt = paths[which[b]][min(start[b] + rng.integers(0, 3), len(paths[which[b]]) - 1)]
        state[b] = [pt[0] + rng.uniform(-0.2, 0.2), pt[1] + rng.uniform(-0.2, 0.2), rng.uniform(0, 9), pt[2] + rng.uniform(-0.1, 0.1)]
    # a short remaining path: the window runs into the end (reaches_end) for some
    ln = np.array([min(len(paths[w]), s + rng.integers(3, 60)) for w, s in zip(which, start)])
    if degenerate is not None:
        which[degenerate], start[degenerate], ln[degenerate] = 3, 0, 12
        state[degenerate] = [2.9, 0.1, 3.0, 0.0]
    uw = np.stack([rng.uniform(-1.5, 1.0, (B, T)), rng.uniform(-0.7, 0.7, (B, T))], axis=1)       # steering beyond the clamp for some
    return dict(paths=paths, table=np.concatenate(paths), off=offs[which], which=which, start=start, ln=ln, state=state, uw=uw)


def _check_prepare(ctx, B, T, seed, degenerate=None, with_ov=False):
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    from oracle import oracle_py as orc
    c = _window_case(B, T, seed, degenerate)
    ctx.set_mpc_params(MpcParams(T=T))
    dl = float(np.linalg.norm(c['paths'][0][0, :2] - c['paths'][0][1, :2]))
    rng = np.random.default_rng(seed + 1)
    x_prev = rng.uniform(-2.0, 9.0, (B, 4, T + 1)) if with_ov else None
    tind = ctx.i32(c['start'])
    out = ctx.prepare(ctx.f64(c['state']), ctx.f64(c['uw']), ctx.f64(c['table']), ctx.i32(c['off']), ctx.i32(c['ln']), dl, tind,
                      x_prev=None if x_prev is None else ctx.f64(x_prev))
    ctx.synchronize()
    got_t, xref, re, xbar = tind.cpu().numpy(), out['xref'].cpu().numpy(), out['reaches_end'].cpu().numpy(), out['xbar'].cpu().numpy()
    po = orc.MpcParams(T=T)
    worst = 0.0
    for b in range(B):
        p = c['paths'][c['which'][b]][:c['ln'][b]]
        wx, ws, wre = orc.calc_ref_trajectory(po, c['state'][b], p[:, 0], p[:, 1], p[:, 2], dl, int(c['start'][b]),
                                              ov=None if x_prev is None else x_prev[b, 2])
        if b == degenerate:
            assert ws < 0 and got_t[b] == -1 and not xref[b].any() and not re[b].any(), (b, ws, got_t[b])
        else:
            assert ws >= 0 and got_t[b] == ws, (B, T, b, got_t[b], ws)
            assert np.array_equal(xref[b], wx) and np.array_equal(re[b], wre), (B, T, b)
        worst = max(worst, float(np.abs(xbar[b] - orc.predict_motion(po, c['state'][b], c['uw'][b, 0], c['uw'][b, 1])).max()))
    print('B = %d, T = %d: max |xbar - oracle| = %.2e' % (B, T, worst))
    assert worst <= TRIG_TOL, (B, T, worst)


@pytest.mark.parametrize('T', [1, 13, 20, 32])
def test_window_and_rollout_of_odd_batches(ctx, T):
    """1, 7 and 65 agents (a window wavefront holds 8, a rollout workgroup 64: one agent, a partly filled wavefront, a last wavefront and a
    last workgroup with one agent) at horizons 1, 13, 20 and 32 (32, 4, 3 and 1 windows per pass; at 32 a window fills more than half a wavefront), through the
    per-stage entry point, where every agent scans its path: target_ind, xref and reaches_end are the oracle's, xbar within 1e-12"""
    for B in (1, 7, 65):
        _check_prepare(ctx, B, T, seed=1000 * T + B)


def test_degenerate_path_in_the_middle_of_a_block(ctx):
    """agent 11 of 21 (the fourth of its wavefront, between two passes' worth of neighbours) has no nearest index: target_ind = -1 and a zero
    window for it, the oracle's windows for everybody around it"""
    _check_prepare(ctx, 21, 20, seed=77, degenerate=11)


def test_window_spaced_by_the_previous_pass(ctx):
    """the second linearisation pass (lin_passes = 2): the window's travel is the cumulative sum of the previous pass's speeds, per lane of
    the agent's run"""
    for T in (13, 20, 32):
        _check_prepare(ctx, 19, T, seed=5 + T, with_ov=True)


# ---- 3. the queue order

@pytest.mark.parametrize('name', ['traffic', 'scene'])
def test_order_is_a_sorted_permutation_of_the_filed_agents(ctx, stock, name):
    """random iteration counts as the queue's hint, three times over: `order` holds every filed agent once -- with retirement ('scene') the
    agents that are not retired -- and their keys never rise along it"""
    sim = FH.build(ctx, stock, name)
    sim.run(FH.BURN_IN)
    rng = np.random.default_rng(3)
    for _ in range(3):
        ctx.synchronize()
        filed = np.arange(sim.P) if sim.done is None else np.flatnonzero(sim.done.cpu().numpy() == 0)
        sim.sol['iters'].copy_(torch.as_tensor(rng.integers(0, 80, sim.P).astype(np.int32)))
        sim.run(1)
        order, keyslot = ctx.closed_loop_queue(sim.P)
        assert 0 < len(filed) and (name != 'scene' or len(filed) < sim.P)
        assert np.array_equal(np.sort(order[:len(filed)]), filed)
        keys = keyslot[order[:len(filed)]] >> 24
        assert (np.diff(keys) <= 0).all() and len(np.unique(keys)) > 3, keys
        assert (sim.snapshot()['status'][filed] == 0).all()
