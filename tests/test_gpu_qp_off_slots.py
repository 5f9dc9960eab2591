"""Lanes and lane groups of the stage solver that are OFF beside ones that are on (csrc/mpcx_qp_stage.h: the row passes run a slot's
rows under the slot's own predicate act[ls], not under a select per row).

tests/test_gpu_qp_sweep_bits.py holds whole launches to recorded bits; in those every wavefront but the last is full.  Here a case's
problems are solved again in launches that leave most of a wavefront without work, and every problem must come out bit for bit as it did
in the full launch -- which is first checked against the recorded digests itself, so the reference is the recorded one:
  1. problem 0 alone: seven drained groups beside it in its wavefront;
  2. the first 9 problems: a full wavefront, and one group beside seven drained ones in the second;
  3. the same 9 with plain rounds switched off (mpcx_qp_set_plain_rounds(ctx, 0)): the generic text of every pass.
A drained group has act = rate = false in every slot, so its rows must stay s = 1, lam = 0 and its lanes must add nothing to what the
wavefront's other groups compute (nothing crosses groups but the ballots).

Cases: the horizon sweep at T = 1 (one stage: rate rows off everywhere, seven lanes off), 3 (SPL = 2, a half-used lane), 17 and 19
(SPL = 3, the last working lane partly off), 20 (the benchmark's shape: lane 6 partly off, lane 7 off) and 25 (SPL = 4, three slots off);
the five-state kernel (T13-jerk-9, and T25-jerk at SPL = 4) and per-problem tuning rows (T20-tuned-8)."""
import numpy as np
import pytest

from tests import qp_bits_helpers as QB

pytestmark = pytest.mark.gpu

CASES = ('sweep-T1', 'sweep-T3', 'sweep-T17', 'sweep-T19', 'sweep-T20', 'sweep-T25', 'T13-jerk-9', 'T20-tuned-8', 'T25-jerk')
# (problems, plain rounds)
PARTS = {'one-problem': (1, True), 'nine-problems': (9, True), 'nine-problems-generic-text': (9, False)}


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.set_qp_plain_rounds(True)
    c.close()


_FULL = {}


def _full(ctx, name):
    """the case and its full launch, solved once and checked against the recorded digests before anything is compared with it"""
    if name not in _FULL:
        want = QB.fixture()['cases'][name]
        case = QB.build(name)
        assert case['arrays'][0].shape[0] == want['problems']
        assert QB.inputs_digest(case) == want['inputs'], 'case %s: the INPUTS differ from the recorded ones (not the solver)' % name
        ctx.set_qp_plain_rounds(True)
        out = QB.solve(ctx, case)
        differing = [k for k in QB.FIELDS if QB.digest(out[k]) != want[k]]
        assert not differing, 'case %s: the full launch differs from the recorded bits in %s' % (name, ', '.join(differing))
        _FULL[name] = (case, out)
    return _FULL[name]


@pytest.mark.parametrize('part', sorted(PARTS))
@pytest.mark.parametrize('name', CASES)
def test_a_problem_beside_drained_groups_comes_out_as_in_the_full_launch(ctx, name, part):
    case, full = _full(ctx, name)
    n, plain = PARTS[part]
    assert case['arrays'][0].shape[0] >= n
    sub = dict(case, arrays=[a[:n] for a in case['arrays']])
    try:
        ctx.set_qp_plain_rounds(plain)
        out = QB.solve(ctx, sub)
    finally:
        ctx.set_qp_plain_rounds(True)
    differing = {k: [int(p) for p in range(n) if not np.array_equal(out[k][p], full[k][p])] for k in QB.FIELDS}
    differing = {k: v for k, v in differing.items() if v}
    print('%s, %s: %d problems, iterations %s; rows differing from the full launch: %s'
          % (name, part, n, out['iters'].tolist(), differing))
    assert all(out[k].shape[0] == n for k in QB.FIELDS)
    assert not differing, 'case %s, %s: problems differing from the full launch, by field: %s' % (name, part, differing)
