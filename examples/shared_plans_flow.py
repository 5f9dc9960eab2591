#!/usr/bin/env python3
"""What connected vehicles change at the crossing: agents seen on their plans instead of on their last controls.

Every agent of the device loop is seen by the others through a prediction of its pool row: the controls it applied in the last step, held
for 35 frames -- the reference's prediction of a scripted car, which has no plan.  An MPC agent does have one: the solution of the step
before, which holds its braking in front of a cut path or a stop line.  IntersectionBatch.share_plans() lets the others see it.

The flagship family -- instances x 8 agents on the eight stock routes, seeded starts -- is run with a share of connected vehicles of 0,
one half (a seeded choice per agent) and 1.  Printed side by side, from the run log: arrivals, the share of agent-steps standing, the mean
speed, contacts and worst clearance.

    python examples/shared_plans_flow.py [--instances 64] [--steps 200] [--horizon 20] [--seed 0] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STOP_SPEED = 0.1389     # lib/mpc.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    print('%d instances x 8 stock routes, T = %d, seeded starts (%d), %d steps' % (args.instances, args.horizon, args.seed, args.steps))
    cols = {}
    for name, frac in (('nobody shares', 0.0), ('half share', 0.5), ('everybody shares', 1.0)):
        sim = synthetic_batch(ctx, B=args.instances, A=8, T=args.horizon, seed=args.seed, routes=routes, dl=dl, cd=cd)
        log = sim.attach_log(args.steps)
        if frac > 0:
            sim.share_plans(np.random.default_rng(args.seed).random(sim.P) < frac)
        ctx.synchronize()
        t0 = time.perf_counter()
        sim.run(args.steps, args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        rows, out = log.rows(), log.outcomes()
        there = out['goal_step'] >= 0
        seen = np.isfinite(out['min_clearance'])
        v = rows['v']
        cols[name] = ('%d of %d' % (0 if sim.share is None else int((sim.share != 0).sum().item()), sim.P),
                      '%d of %d' % (int(there.sum()), sim.P), '%.1f %%' % (100.0 * float((np.abs(v) <= STOP_SPEED).mean())),
                      '%.3f m/s' % float(v.mean()), '%d' % int((out['contact_step'] >= 0).sum()),
                      '%.2f m' % (float(out['min_clearance'][seen].min()) if seen.any() else float('inf')), '%.2f s' % wall)
    names = list(cols)
    print('%-36s' % '' + ''.join('%20s' % n for n in names))
    for i, what in enumerate(('connected vehicles', 'cars that reached their goal', 'agent-steps standing', 'mean speed', 'cars with a contact',
                              'worst clearance', 'wall time')):
        print('%-36s' % what + ''.join('%20s' % cols[n][i] for n in names))


if __name__ == '__main__':
    main()
