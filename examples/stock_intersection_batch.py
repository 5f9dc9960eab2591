#!/usr/bin/env python3
"""The reference's stock scenario (main/scenarios/mpc_intersection.py: one ego, two scripted cars that never yield) x B, advanced on
the device in ONE call: the scripted cars are stepped by a HIP kernel (mpcx_traffic_step_batch inside mpcx_closed_loop_run), no host work
between steps.  Instance 0 is the stock set itself (ego route (4, 1); cars: direction 1 / offset 2 s / straight on and direction -1 /
offset 4 s / turning, 25 km/h); the others draw route, directions, turning, speeds and start delays (batch.scripted_traffic_batch).
A run log with capacity 0 (attach_log: the per-ego outcomes only, 24 bytes per ego) says what the reference's loop says about a run: when
mpc.is_goal held (the reference's loop ends there), whether anybody touched anybody after having been clear, and the worst clearance.
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
    log = sim.attach_log(0)                 # outcomes only: goal arrival, contact, worst clearance -- written on the device, step by step
    sim.run(1, graph=args.graph)            # first call: allocations (and the capture)
    ctx.synchronize()
    t0 = time.perf_counter()
    sim.run(args.steps - 1, graph=args.graph)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    sim.check()
    snap = sim.snapshot()
    path_len = sim.path_len.cpu().numpy()
    out = log.outcomes()
    arrived = out['goal_step'] >= 0         # mpc.is_goal held: the reference's loop would have ended after goal_step iterations
    under_way = ~arrived                    # an arrived ego stands at its goal: "standing" and "mean speed" are about the others
    v = snap['state'][under_way, 2]
    touched = out['contact_step'] >= 0      # clearance < 0 after the ego had been clear of everybody (a car may spawn ON an ego)
    seen = np.isfinite(out['min_clearance'])
    stats = ctx.closed_loop_stats()
    print('%d instances x %d steps on the device: %.0f instance-steps/s (%.3f ms per step); %d of %d egos arrived (median after %s steps), '
          'of the others %d are standing, mean speed %.2f m/s; %d egos touched a vehicle, worst clearance %.2f m; %d QP failures; '
          'stock instance: arrived after %d steps, ego at path point %d of %d, cars at x = %s'
          % (args.instances, args.steps, args.instances * (args.steps - 1) / wall, 1e3 * wall / max(args.steps - 1, 1), int(arrived.sum()),
             len(arrived), int(np.median(out['goal_step'][arrived])) if arrived.any() else '-', int((np.abs(v) < 0.1).sum()),
             float(v.mean()) if len(v) else 0.0, int(touched.sum()), float(out['min_clearance'][seen].min()) if seen.any() else float('inf'),
             stats['failures'], int(out['goal_step'][0]), int(snap['traj_idx'][0]), int(path_len[0]),
             np.round(snap['traffic_state'][:2, 0], 2).tolist()))


if __name__ == '__main__':
    main()
