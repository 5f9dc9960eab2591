"""Record tests/golden/qp_stage_exit_bits.json: per case of tests/qp_exit_helpers.py (sixteen problems per launch: five shapes, each with
stock parameters, a low iteration cap, a loose tolerance, two infeasible starts and every parameter moved) the SHA-256 of the raw bytes of
u, x, status, iters and kkt as the stage-structured QP solver returns them, on the build this script is run with.
tests/test_gpu_qp_exit_bits.py holds every later build to these digests.

    python scripts/record_qp_exit_bits.py --commit <the commit the build is of> [--out tests/golden/qp_stage_exit_bits.json]

Run it on the PARENT of a change that must not move a bit of the solver's results (MPCX_LIB may point at that build's libmpcx.so).

The sixteen problems of a shape are the first sixteen of its pool, unless those hold no problem that the trial pass accepts or none that
polishes under stock parameters: then the pool's first such problem takes the place of the last (second to last) of the sixteen.  The
rows are written into the fixture.  The script also solves every case the two other ways the test does (behind a launch with other
parameters, tiled into a refilling launch) and says whether this build gives the recorded bits there as well."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def choose_rows(QE, ctx, shape):
    from tests import test_gpu_qp_plain_round as PR
    probs = QE.pool(shape)
    case = dict(params=QE.stock(shape), arrays=PR._stack(probs, QE.stock(shape).T), tuned=shape == 'T20-tuned')
    out = QE.launch(ctx, case)
    trial, pol = np.nonzero(QE.by_trial(out))[0].tolist(), np.nonzero(QE.polished(out))[0].tolist()
    print('%-10s pool of %d: %d accepted by the trial pass, %d polish, statuses %s' % (shape, len(probs), len(trial), len(pol),
                                                                                      sorted(set(out['status'].tolist()))), flush=True)
    rows = list(range(QE.N))
    if trial and not set(trial) & set(rows):
        rows[QE.N - 1] = trial[0]
    if pol and not set(pol) & set(rows[:QE.N - 1]):
        rows[QE.N - 2] = pol[0]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit whose stage solver this build has')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'qp_stage_exit_bits.json'))
    args = ap.parse_args()
    from mpc_for_av_at_intersection_amd.runtime import Context
    from tests import qp_exit_helpers as QE
    ctx = Context(0)
    rows = {shape: choose_rows(QE, ctx, shape) for shape in QE.SHAPES}
    cases, outs, unstable = {}, {}, []
    for name in QE.CASES:
        case = QE.build(name, rows[name.split('/')[0]])
        out = outs[name] = QE.launch(ctx, case)
        cases[name] = QE.record(out, case)
        QE.launch(ctx, QE.other(case))
        again = QE.launch(ctx, case)
        tiled, copies = QE.refilling(ctx, case, out)
        late = [k for k in QE.FIELDS if not np.array_equal(again[k], out[k])]
        refill = [k for k in QE.FIELDS if any(not np.array_equal(tiled[k][c * QE.N:(c + 1) * QE.N], out[k]) for c in range(copies))]
        if late or refill:
            unstable.append(name)
        print('%-12s statuses %s, iterations %s, trial %d, polished %d; differing behind other parameters: %s; in %d tiled copies: %s'
              % (name, out['status'].tolist(), out['iters'].tolist(), cases[name]['by_trial'], cases[name]['polished'], late, copies, refill), flush=True)
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump({'recorded_at_commit': args.commit, 'fields': list(QE.FIELDS), 'rows': rows, 'cases': cases}, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d cases' % (args.out, len(cases)))
    seen = set(s for c in cases.values() for s in c['statuses'])
    assert {0, 1, 2} <= seen, 'the recorded statuses %s lack OPTIMAL (0), the iteration cap (1) or the infeasible start (2)' % sorted(seen)
    for shape in QE.SHAPES:
        a = outs[shape + '/a']
        assert QE.by_trial(a).any() and QE.polished(a).any(), 'shape %s: no problem accepted by the trial pass, or none that polishes' % shape
    assert not unstable, 'this build does not repeat its own bits in %s' % unstable


if __name__ == '__main__':
    main()
