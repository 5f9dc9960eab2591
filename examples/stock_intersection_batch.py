#!/usr/bin/env python3
"""The reference's stock scenario (main/scenarios/mpc_intersection.py: one ego, two scripted cars that never yield) x B, advanced on
the device in ONE call: the scripted cars are stepped by a HIP kernel (mpcx_traffic_step_batch inside mpcx_closed_loop_run), no host work
between steps.  Instance 0 is the stock set itself (ego route (4, 1); cars: direction 1 / offset 2 s / straight on and direction -1 /
offset 4 s / turning, 25 km/h); the others draw route, directions, turning, speeds and start delays (batch.scripted_traffic_batch).
examples/stock_intersection.py is the same scenario, one instance, through the reference's call surface.

    python examples/stock_intersection_batch.py [--instances 1024] [--steps 120] [--horizon 20] [--graph]
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
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    sim = scripted_traffic_batch(ctx, B=args.instances, T=args.horizon, seed=args.seed, A=1, K=2)
    sim.run(1, graph=args.graph)            # first call: allocations (and the capture)
    ctx.synchronize()
    t0 = time.perf_counter()
    sim.run(args.steps - 1, graph=args.graph)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    sim.check()
    snap = sim.snapshot()
    path_len = sim.path_len.cpu().numpy()
    # an ego has passed once it is beyond the junction: in the last fifth of its path (the batch has no goal test: egos stand at the path end)
    passed = snap['traj_idx'] >= 0.8 * path_len
    stats = ctx.closed_loop_stats()
    print('%d instances x %d steps on the device: %.0f instance-steps/s (%.3f ms per step); %d of %d egos passed the junction, '
          '%d are standing, mean speed %.2f m/s; %d QP failures; stock instance: ego at path point %d of %d, cars at x = %s'
          % (args.instances, args.steps, args.instances * (args.steps - 1) / wall, 1e3 * wall / max(args.steps - 1, 1), int(passed.sum()),
             len(passed), int((np.abs(snap['state'][:, 2]) < 0.1).sum()), float(snap['state'][:, 2].mean()), stats['failures'],
             int(snap['traj_idx'][0]), int(path_len[0]), np.round(snap['traffic_state'][:2, 0], 2).tolist()))


if __name__ == '__main__':
    main()
