#!/usr/bin/env python3
"""How many vehicles per hour does the controller put through the crossing at a given demand, and how long do they queue?

The eight stock routes are eight SLOTS; every slot serves a stream of vehicles (IntersectionBatch.respawn_on_schedule).  The two routes of an
approach arm share their first point, so every arm is one queue fed by one seeded memoryless arrival stream (batch.demand_schedule) that is
dealt to the arm's two slots in turn.  A vehicle enters in its due step or the first later step in which its slot is free and its start pose
is `--gap` metres clear; when it arrives, its episode is recorded and the slot is reset for the next vehicle -- all on the device, with no
host work between the steps.  The sweep runs one batch per mean headway and reads everything from episodes().

    python examples/intersection_throughput.py [--instances 64] [--headways 60,30,15,8] [--vehicles 4] [--gap 2.0] [--max-steps 2000]
                                               [--chunk 32] [--horizon 13] [--seed 0] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=64)
    ap.add_argument('--headways', default='60,30,15,8', help='mean headways of an approach queue in steps (each >= 1), comma-separated')
    ap.add_argument('--vehicles', type=int, default=4, help='vehicles per slot (two slots per approach arm)')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a vehicle needs at its start pose to be let in')
    ap.add_argument('--max-steps', type=int, default=2000)
    ap.add_argument('--chunk', type=int, default=32, help='steps between two looks at the number of agents driving or waiting')
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    print('%d instances x 8 slots x %d vehicles, gap %.1f m, seed %d' % (args.instances, args.vehicles, args.gap, args.seed))
    print('%8s %8s %8s %12s %12s %10s %9s %10s' % ('headway', 'steps', 'served', 'veh/h', 'mean delay', 'max delay', 'contacts', 'clearance'))
    for headway in (float(h) for h in args.headways.split(',')):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        due = demand_schedule(route, routes, np.zeros_like(route), headway, args.vehicles, args.seed)
        sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap)
        ctx.synchronize()
        t0 = time.perf_counter()
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        ep = sim.episodes()
        # the demand is over when the last vehicle has arrived: throughput over that span of simulated time, per instance
        span_h = (int(ep['arrived'].max()) + 1) * sim.params.dt / 3600.0 if len(ep) else float('nan')
        seen = np.isfinite(ep['min_clearance'])
        print('%8.1f %8d %8d %12.0f %10.1f s %8.1f s %9d %8.2f m   (%.2f s wall)'
              % (headway, taken, len(ep), len(ep) / args.instances / span_h, float(ep['delay'].mean()) * sim.params.dt,
                 float(ep['delay'].max()) * sim.params.dt, int(ep['contact'].sum()), float(ep['min_clearance'][seen].min()) if seen.any() else float('inf'),
                 wall))


if __name__ == '__main__':
    main()
