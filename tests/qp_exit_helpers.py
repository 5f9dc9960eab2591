"""Launches of sixteen problems through the stage-structured QP solver at its exits, held to recorded bits
(tests/golden/qp_stage_exit_bits.json).  Shared by scripts/record_qp_exit_bits.py (which writes the fixture) and
tests/test_gpu_qp_exit_bits.py (which compares with it).  Digests and the way a launch is described are those of tests/qp_bits_helpers.py.

A case is SHAPE/VARIANT.  The shapes: T20 (three slots per lane), T3 (two, the second lane half used), T25 (four), T13-jerk (the
five-state kernel) and T20-tuned (per-problem tuning rows).  The variants:
  a  stock parameters
  b  max_iter = 3 (the iteration-cap exit)
  c  tol = 1e-3 (a loose tolerance: the convergence test passes one to three iterations earlier)
  d  the speed of two of the sixteen initial states beyond max_speed (the infeasible-start exit)
  e  every field of the parameters moved off its stock value by a few per cent (T and model select the kernel and stay).  The four
     uniform shapes run the kernel without tuning rows; T20-tuned takes the moved set as launch parameters AND as its tuning rows.
In every variant the rows of T20-tuned repeat the launch parameters, so its recorded bits equal T20's: the shape checks that the kernel with
tuning rows reproduces the uniform one at the exits, NOT whether a field came from the row or from the launch (no case has rows that differ
from the launch parameters; tests/test_gpu_tuning.py is where rows differ).
The sixteen problems of a shape are rows of a pool (POOLS); which rows is written in the fixture by the recording script."""
import dataclasses
import os

import numpy as np

from tests import helpers as H
from tests import qp_bits_helpers as QB

FIXTURE = os.path.join(H.GOLD, 'qp_stage_exit_bits.json')
FIELDS = QB.FIELDS
SHAPES = ('T20', 'T3', 'T25', 'T13-jerk', 'T20-tuned')
VARIANTS = ('a', 'b', 'c', 'd', 'e')
CASES = tuple('%s/%s' % (s, v) for s in SHAPES for v in VARIANTS)
N = 16
INFEASIBLE_ROWS = (3, 11)       # variant d: positions within the sixteen

# corpus rows at T = 20: the polish hand-over set and the longest solves of tests/test_gpu_qp_plain_round.py, then rows the trial pass accepts
_T20_POOL = (158, 0, 238, 1, 4, 3, 134, 142) + tuple(range(321, 332)) + tuple(range(5, 34))


def _fixture():
    import json
    with open(FIXTURE) as f:
        return json.load(f)


_pools = {}


def pool(shape):
    """the candidate problems of a shape: a list of (x0, xref, xbar, re, u_warm)"""
    if shape not in _pools:
        from tests import test_gpu_qp_plain_round as PR
        from tests.test_oracle_jerk import jerk_cases
        if shape in ('T20', 'T20-tuned'):
            rows = PR._corpus_rows(_T20_POOL)
        elif shape == 'T13-jerk':
            rows = jerk_cases(13)[:48]
        else:
            rows = H.horizon_problems(int(shape[1:]), n=24)[:48]
        _pools[shape] = rows
    return _pools[shape]


def stock(shape):
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    if shape == 'T13-jerk':
        return MpcParams.jerk(T=13)
    return MpcParams(T=int(shape.split('-')[0][1:]))


def moved(p, sign=1.0):
    """every field of p but T and model a few per cent off (a different amount per field; sign = -1: off to the other side)"""
    k = [0]

    def f(v):
        k[0] += 1
        m = 0.01 * (2 + k[0] % 4)
        return v * (1.0 + sign * m) if v != 0.0 else m      # (a zero weight becomes a small positive one)

    seq = lambda v: tuple(f(x) for x in v)
    return dataclasses.replace(p, dt=f(p.dt), L=f(p.L), w_perp=f(p.w_perp), w_para=f(p.w_para), R=seq(p.R), Rd=seq(p.Rd), Q_v_yaw=seq(p.Q_v_yaw),
                               Qf_base=seq(p.Qf_base), R_end=seq(p.R_end), max_speed=f(p.max_speed), min_speed=f(p.min_speed),
                               max_accel=f(p.max_accel), max_decel=f(p.max_decel), max_steer=f(p.max_steer), max_dsteer=f(p.max_dsteer),
                               max_iter=p.max_iter - 3 if p.max_iter > 10 else p.max_iter + 2, tol=f(p.tol), jerk_weight=f(p.jerk_weight))


def build(name, rows):
    """the launch of a case from the pool rows of its shape: dict(params, arrays, tuned), as tests/qp_bits_helpers.py::build"""
    from tests import test_gpu_qp_plain_round as PR
    shape, variant = name.split('/')
    p = stock(shape)
    probs = [pool(shape)[k] for k in rows]
    assert len(probs) == N
    arrays = PR._stack(probs, p.T)
    if variant == 'b':
        p = dataclasses.replace(p, max_iter=3)
    elif variant == 'c':
        p = dataclasses.replace(p, tol=1e-3)
    elif variant == 'd':
        arrays[0] = arrays[0].copy()
        for k in INFEASIBLE_ROWS:
            arrays[0][k, 2] = p.max_speed + 1.0
    elif variant == 'e':
        p = moved(p)
    return dict(params=p, arrays=arrays, tuned=shape == 'T20-tuned')


def other(case):
    """the same problems under different uniform parameters (moved to the other side): the launch in front of a case's second solve"""
    return dict(case, params=moved(case['params'], -1.0), tuned=False)


def launch(ctx, case, arrays=None, hint=None):
    """one launch through the stage solver into pre-filled outputs (a row that is not written shows)"""
    import torch
    p = case['params']
    a = case['arrays'] if arrays is None else arrays
    B, T, f = a[0].shape[0], p.T, torch.float64
    out = dict(x=torch.full((B, 4, T + 1), float('nan'), dtype=f, device=ctx.device), u=torch.full((B, 2, T), float('nan'), dtype=f, device=ctx.device),
               status=torch.full((B,), -77, dtype=torch.int32, device=ctx.device), iters=torch.full((B,), -77, dtype=torch.int32, device=ctx.device),
               kkt=torch.full((B, 4), float('nan'), dtype=f, device=ctx.device))
    ctx.set_mpc_params(p)
    ctx.set_qp_solver('stage')
    try:
        if case['tuned']:
            ctx.set_instance_tuning(ctx.f64(np.tile(p.tuning_row(), (B, 1))))
        ctx.set_qp_order_hint(None if hint is None else ctx.i32(hint))
        ctx.qp_solve(ctx.f64(a[0]), ctx.f64(a[1]), ctx.f64(a[2]), ctx.u8(a[3]), ctx.f64(a[4]), out=out)
        ctx.synchronize()
    finally:
        ctx.set_qp_order_hint(None)
        ctx.set_instance_tuning(None)
        ctx.set_qp_solver('auto')
    return {k: out[k].cpu().numpy() for k in FIELDS}


def refilling(ctx, case, sixteen):
    """the sixteen problems tiled past the lane groups that are resident in one launch (8 x 4 x CUs) and handed out easiest first, as
    tests/test_gpu_qp_refill_order.py builds its third launch: groups draw copies of them behind finished problems.  Returns the outputs
    and the number of copies."""
    import torch
    groups = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    copies = -(-(groups + 4 * N) // N)
    arrays = [np.tile(a, (copies,) + (1,) * (a.ndim - 1)) for a in case['arrays']]
    hint = np.tile((63 - np.clip(sixteen['iters'], 0, 63)).astype(np.int32), copies)
    return launch(ctx, case, arrays, hint), copies


def polished(out):
    """problems that went through a polish round.  Every exit test that ends a solve (converged, reduced accuracy, iteration cap) first
    sends the group into a polish round of that iterate (solve_queue: `(stop_ok || stop_fail) && ptested != it`), so a problem that
    ended OPTIMAL after at least one iteration has polished; the trial pass (0 iterations) and an infeasible start have not."""
    return (out['status'] == 0) & (out['iters'] >= 1)


def by_trial(out):
    return (out['status'] == 0) & (out['iters'] == 0)


def record(out, case):
    rec = {'inputs': QB.inputs_digest(case), 'statuses': sorted(set(out['status'].tolist())), 'max_iters': int(out['iters'].max()),
           'by_trial': int(by_trial(out).sum()), 'polished': int(polished(out).sum())}
    rec.update({k: QB.digest(out[k]) for k in FIELDS})
    return rec
