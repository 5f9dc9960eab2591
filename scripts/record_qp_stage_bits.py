"""Record tests/golden/qp_stage_bits.json: per case of tests/qp_bits_helpers.py the SHA-256 of the raw bytes of u, x, status, iters and kkt as
the stage-structured QP solver returns them, on the build this script is run with.  tests/test_gpu_qp_sweep_bits.py holds every later build
to these digests.

    python scripts/record_qp_stage_bits.py --commit <the commit the build is of> [--out tests/golden/qp_stage_bits.json]

Run it on the PARENT of a change that must not move a bit of the solver's results (MPCX_LIB may point at that build's libmpcx.so).  Record
again only with a change that is allowed to move bits, and say so in that change."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit whose stage solver this build has')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'qp_stage_bits.json'))
    args = ap.parse_args()
    from mpc_for_av_at_intersection_amd.runtime import Context
    from tests import qp_bits_helpers as QB
    ctx = Context(0)
    cases = {}
    for name in QB.CASES:
        cases[name] = QB.record(ctx, name)
        print('%-26s %3d problems, iterations up to %2d, status != 0: %d' % (name, cases[name]['problems'], cases[name]['max_iters'],
                                                                             cases[name]['status_nonzero']), flush=True)
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump({'recorded_at_commit': args.commit, 'fields': list(QB.FIELDS), 'cases': cases}, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d cases' % (args.out, len(cases)))


if __name__ == '__main__':
    main()
