#!/usr/bin/env python3
"""The two ways the reference makes an ego yield to a crossing car, for the SAME seeded family of instances (one ego, two scripted cars
that never yield; batch.scripted_traffic_batch), each advanced on the device in one call:

  cut    main/scenarios/mpc_intersection.py: the path is cut in front of the conflict, the MPC runs into the path end
  speed  main/scenarios/mpc_intersection_new_ref.py + lib/mpc_with_speed.py: the path stays whole and the speed reference (tracked with
         weight 20) is zeroed from the conflict on -- IntersectionBatch(..., stop_mode='speed')

Both with the controller constants of lib/mpc_with_speed.py (lib.mpc_with_speed.params), so that the stop mode is the only difference.
A run log with capacity 0 (the per-ego outcomes only) says what the reference's loop says about a run: when mpc.is_goal held, whether
anybody touched anybody after having been clear, and the worst clearance.  examples/stock_intersection_batch.py is the stock script alone.

    python examples/speed_reference_intersection_batch.py [--instances 1024] [--steps 120] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=120)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, stock_routes
    from mpc_for_av_at_intersection_amd.lib import mpc_with_speed
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    params = mpc_with_speed.params(cd, 0.2)
    for mode in ('cut', 'speed'):
        sim = scripted_traffic_batch(ctx, B=args.instances, seed=args.seed, A=1, K=2, routes=routes, dl=dl, cd=cd, mpc=params, stop_mode=mode)
        log = sim.attach_log(0)
        sim.run(1, graph=args.graph)            # first call: allocations (and the capture)
        ctx.synchronize()
        t0 = time.perf_counter()
        sim.run(args.steps - 1, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        out = log.outcomes()
        arrived = out['goal_step'] >= 0
        touched = out['contact_step'] >= 0
        seen = np.isfinite(out['min_clearance'])
        v = sim.snapshot()['state'][~arrived, 2]
        stats = ctx.closed_loop_stats()
        print('%-5s %d instances x %d steps: %.0f instance-steps/s; %d of %d egos arrived (median after %s steps), of the others %d are '
              'standing; %d egos touched a vehicle, worst clearance %.2f m, median %.2f m; %d QP failures'
              % (mode, args.instances, args.steps, args.instances * (args.steps - 1) / wall, int(arrived.sum()), len(arrived),
                 int(np.median(out['goal_step'][arrived])) if arrived.any() else '-', int((np.abs(v) < 0.1).sum()), int(touched.sum()),
                 float(out['min_clearance'][seen].min()) if seen.any() else float('inf'),
                 float(np.median(out['min_clearance'][seen])) if seen.any() else float('inf'), stats['failures']))
        del sim, log
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
