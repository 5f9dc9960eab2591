"""Plain copies of the stage solver's row passes against the generic text (csrc/mpcx_qp_stage.h, mpcx_qp_set_plain_rounds).

The device build has second copies of the predictor's row pass (C) and of the corrector's row pass (D), compiled with the trial / polish
flags folded, and runs them in the rounds in which no problem of the wavefront is in a trial or polish round.  With
the switch off every round runs the generic text.  Every launch here is solved with the switch on and off and must come out bit for bit
the same in x, u, status, iters and kkt: that compares copy against copy for every problem, whatever its neighbours in the wavefront
do (tests/test_gpu_qp_plain_round.py compares two arrangements of a launch instead, which leaves the comparison to chance).

With the switch on the iteration counts are those of the solver from before it had plain rounds (tests/golden/qp_plain_round_iters.json)
and the solutions are within 2e-7 of the oracle, the bar of tests/test_gpu_parity.py.

Covered: SPL = 2 (T10-9, T13-jerk-9), 3 (everything at T = 20) and 4 (T28-9, T25-jerk), the five-state problem (T13-jerk-9, and T25-jerk:
the SPL = 4 five-state kernel, the instantiation that went wrong when the residual pass had a copy too) and per-problem tuning rows
(T20-tuned-8).

What these comparisons cannot show: that the switch reaches the kernel at all.  Both settings give the same bits by design, so a launch
that ignored the switch would pass every comparison here; nothing observable from outside tells the two texts apart.  That the flag is
carried (QpArgs.plain_rounds, and the key of the closed loop's captured graph) is a matter of reading the code, and no test drives the
switch through mpcx_closed_loop_run.

NOT covered: the entry into polish at an exit test (pinit).  No problem of the corpus, of the golden sets or of
qp_hard / qp_hard2 takes it (see tests/test_gpu_qp_plain_round.py), and no failing input is constructed for it."""
import numpy as np
import pytest

from tests import test_gpu_qp_plain_round as PR

pytestmark = pytest.mark.gpu

FIELDS = PR.FIELDS


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.set_qp_plain_rounds(True)
    c.close()


def _both(ctx, case, hint=None):
    """the launch with plain rounds (the default) and with the generic text only"""
    try:
        ctx.set_qp_plain_rounds(True)
        on = PR.solve(ctx, case, hint)
        ctx.set_qp_plain_rounds(False)
        off = PR.solve(ctx, case, hint)
    finally:
        ctx.set_qp_plain_rounds(True)
    return on, off


def _same_bits(on, off, what):
    differing = [k for k in FIELDS if not np.array_equal(on[k], off[k])]
    print('%s: %d problems, iterations up to %d; fields differing between switch on and off: %s'
          % (what, len(on['iters']), int(on['iters'].max()), differing))
    assert not differing, differing


def _corpus_iters():
    rec = PR.parent_iters()
    return [it for k in range(6) for it in rec['T20-corpus-%d' % k]]


def _plain_case(rows, T=20):
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    return dict(params=MpcParams(T=T), arrays=PR._stack(rows, T), tuned=False)


@pytest.fixture(scope='module')
def corpus():
    """the whole committed corpus as one launch, and the oracle's solutions of its problems (computed once)"""
    from oracle import oracle_py as orc
    rows = PR._corpus_rows(range(377))
    po = orc.MpcParams(T=20)
    ref = [orc.qp_solve(po, r[0], r[1], r[2], r[3], r[4]) for r in rows]
    return _plain_case(rows), ref


def test_corpus_switch_on_and_off_give_the_same_bits(ctx, corpus):
    case, ref = corpus
    on, off = _both(ctx, case)
    _same_bits(on, off, 'corpus, queue as it lies')
    # the counts of the solver from before plain rounds (recorded in chunks of 64), the oracle's solutions to 2e-7 on u and x
    assert (on['status'] == 0).all()
    assert on['iters'].tolist() == _corpus_iters()
    du = max(float(np.abs(r.u - on['u'][k]).max()) for k, r in enumerate(ref))
    dx = max(float(np.abs(r.x[:4] - on['x'][k]).max()) for k, r in enumerate(ref))
    print('corpus: |gpu - oracle| u %.2e x %.2e' % (du, dx))
    assert du < PR.QP_TOL and dx < PR.QP_TOL


def test_corpus_hardest_first_switch_on_and_off_give_the_same_bits(ctx, corpus):
    """the corpus laid out hardest first and handed out as it lies, eight hard problems to a wavefront: plain rounds dominate
    (arrangement A of tests/test_gpu_qp_plain_round.py)"""
    case, _ = corpus
    iters = np.array(_corpus_iters())
    order = np.argsort(-iters, kind='stable')
    sorted_case = dict(case, arrays=[a[order] for a in case['arrays']])
    on, off = _both(ctx, sorted_case)
    _same_bits(on, off, 'corpus, hardest first')
    assert on['iters'].tolist() == iters[order].tolist()


def test_golden_and_hard_problems_switch_on_and_off_give_the_same_bits(ctx):
    from oracle import oracle_py as orc
    rows = PR._golden_rows(20) + PR._hard_rows()
    case = _plain_case(rows)
    on, off = _both(ctx, case)
    _same_bits(on, off, '60 golden problems at T = 20, qp_hard, qp_hard2')
    assert (on['status'] == 0).all()
    assert on['iters'].tolist() == PR.parent_iters()['T20-golden-64'][:62]      # (that record ends with two corpus problems)
    po = orc.MpcParams(T=20)
    ref = [orc.qp_solve(po, r[0], r[1], r[2], r[3], np.zeros((2, 20)) if r[4] is None else r[4]) for r in rows]
    assert all(r.status == 0 for r in ref)
    du = max(float(np.abs(r.u - on['u'][k]).max()) for k, r in enumerate(ref))
    dx = max(float(np.abs(r.x[:4] - on['x'][k]).max()) for k, r in enumerate(ref))
    print('golden + hard: |gpu - oracle| u %.2e x %.2e' % (du, dx))
    assert du < PR.QP_TOL and dx < PR.QP_TOL


def test_five_state_long_horizon_switch_on_and_off_give_the_same_bits(ctx):
    """T = 25, five states: SPL = 4 with the seven-state sweeps (real windows made at T, as tests/test_gpu_horizons.py takes them)"""
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    from oracle import oracle_py as orc
    from tests import helpers as H
    T = 25
    rows = H.horizon_problems(T, n=16)
    case = dict(params=MpcParams.jerk(T=T), arrays=PR._stack(rows, T), tuned=False)
    on, off = _both(ctx, case)
    _same_bits(on, off, 'T25-jerk')
    po = orc.MpcParams.jerk(T=T)
    ref = [orc.qp_solve(po, r[0], r[1], r[2], r[3], np.zeros((2, T)) if r[4] is None else r[4]) for r in rows]
    assert (on['status'] == 0).all() and all(r.status == 0 for r in ref)
    du = max(float(np.abs(r.u - on['u'][k]).max()) for k, r in enumerate(ref))
    dx = max(float(np.abs(r.x[:4] - on['x'][k]).max()) for k, r in enumerate(ref))
    print('T25-jerk: %d problems, |gpu - oracle| u %.2e x %.2e' % (len(rows), du, dx))
    assert du < PR.QP_TOL and dx < PR.QP_TOL


@pytest.mark.parametrize('name', ['T10-9', 'T28-9', 'T13-jerk-9', 'T20-tuned-8'])
def test_other_instantiations_switch_on_and_off_give_the_same_bits(ctx, name):
    """SPL = 2 and 4, the five-state problem and per-problem tuning rows, as tests/test_gpu_qp_plain_round.py builds them"""
    case = PR.build(name)
    n = case['n']
    on, off = _both(ctx, case)
    _same_bits(on, off, name)
    assert (on['status'] == 0).all()
    assert on['iters'][:n].tolist() == PR.parent_iters()[name]
    du = max(float(np.abs(r.u - on['u'][k]).max()) for k, r in enumerate(case['ref']))
    dx = max(float(np.abs(r.x[:4] - on['x'][k]).max()) for k, r in enumerate(case['ref']))
    print('%s: |gpu - oracle| u %.2e x %.2e' % (name, du, dx))
    assert du < PR.QP_TOL and dx < PR.QP_TOL
