"""Launches of the stage-structured QP solver whose outputs are held to recorded bits (tests/golden/qp_stage_bits.json): the cases, how they
are solved and how an output is digested.  Shared by scripts/record_qp_stage_bits.py (which writes the fixture) and
tests/test_gpu_qp_sweep_bits.py (which compares with it), so that both see the same inputs."""
import hashlib
import json
import os

import numpy as np

from tests import helpers as H

FIXTURE = os.path.join(H.GOLD, 'qp_stage_bits.json')
FIELDS = ('u', 'x', 'status', 'iters', 'kkt')
# the horizon sweep: one, two and three slots beyond the horizon, none at all, a single turn and all eight turns, in each of SPL = 2
# (T <= 16: T = 1 one slot of 2 and one turn, 2 none and one turn, 3, 5, 15 one slot, 16 none and eight turns), SPL = 3 (T <= 24: 17 one slot,
# 19 two, 20 one, 21 none, 23 one, 24 none and eight turns) and SPL = 4 (25 three slots, 27 one, 31 one and eight turns, 32 none)
SWEEP_TS = (1, 2, 3, 5, 15, 16, 17, 19, 20, 21, 23, 24, 25, 27, 31, 32)
OTHER = ('T10-9', 'T28-9', 'T13-jerk-9', 'T20-tuned-8')
CASES = ('T20-corpus', 'T20-corpus-hardest-first', 'T20-golden-hard') + OTHER + ('T25-jerk',) + tuple('sweep-T%d' % T for T in SWEEP_TS)


def build(name):
    """the launch of a case, as tests/test_gpu_qp_plain_round.py::solve takes it: dict(params, arrays, tuned)"""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    from tests import test_gpu_qp_plain_round as PR
    if name.startswith('T20-corpus'):
        arrays = PR._stack(PR._corpus_rows(range(377)), 20)
        if name == 'T20-corpus-hardest-first':
            rec = PR.parent_iters()
            iters = np.array([it for k in range(6) for it in rec['T20-corpus-%d' % k]])
            order = np.argsort(-iters, kind='stable')
            arrays = [a[order] for a in arrays]
        return dict(params=MpcParams(T=20), arrays=arrays, tuned=False)
    if name == 'T20-golden-hard':
        return dict(params=MpcParams(T=20), arrays=PR._stack(PR._golden_rows(20) + PR._hard_rows(), 20), tuned=False)
    if name in OTHER:
        case = PR.build(name)
        return dict(params=case['params'], arrays=case['arrays'], tuned=case['tuned'])
    if name == 'T25-jerk':
        return dict(params=MpcParams.jerk(T=25), arrays=PR._stack(H.horizon_problems(25, n=16), 25), tuned=False)
    if name.startswith('sweep-T'):
        T = int(name[len('sweep-T'):])
        rows = H.horizon_problems(T, n=32)[:64]        # two problems per golden case, as two steps of a closed loop
        return dict(params=MpcParams(T=T), arrays=H.stack_problems(rows), tuned=False)
    raise KeyError(name)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs_digest(case):
    h = hashlib.sha256()
    for a in case['arrays']:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def solve(ctx, case):
    """one launch, stage solver forced (mpcx_set_qp_solver(ctx, 2)), the queue handing the problems out as they lie"""
    from tests import test_gpu_qp_plain_round as PR
    return PR.solve(ctx, case, None)


def record(ctx, name):
    case = build(name)
    out = solve(ctx, case)
    rec = {'problems': int(case['arrays'][0].shape[0]), 'inputs': inputs_digest(case),
           'max_iters': int(out['iters'].max()), 'status_nonzero': int((out['status'] != 0).sum())}
    rec.update({k: digest(out[k]) for k in FIELDS})
    return rec


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
