#!/usr/bin/env python3
"""What right of way does to an intersection near capacity.

The open intersection of examples/intersection_throughput.py -- the eight stock routes as eight slots, two per approach arm, every arm one
queue fed by a seeded memoryless arrival stream -- at a SHORT mean headway, run twice on the same demand: once with the reference's rule,
under which every car yields to every other car and cars that meet at the crossing wait for each other, and once with
IntersectionBatch.give_way('entry'): first come, first served -- a car sees the cars that entered the scene after it as standing cars at
their present pose.  Printed side by side: vehicles served, mean queueing delay, contacts and worst clearance (true clearance, from the run
log's outcome words, in both columns).

    python examples/right_of_way_flow.py [--instances 64] [--headway 8] [--vehicles 4] [--gap 2.0] [--max-steps 1200] [--chunk 32]
                                         [--horizon 13] [--seed 0] [--graph]
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
    ap.add_argument('--headway', type=float, default=8.0, help='mean headway of an approach queue in steps (>= 1)')
    ap.add_argument('--vehicles', type=int, default=4, help='vehicles per slot (two slots per approach arm)')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a vehicle needs at its start pose to be let in')
    ap.add_argument('--max-steps', type=int, default=1200)
    ap.add_argument('--chunk', type=int, default=32)
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
    total = args.instances * 8 * args.vehicles
    print('%d instances x 8 slots x %d vehicles = %d, mean headway %.1f steps, gap %.1f m, seed %d, at most %d steps'
          % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps))
    cols = {}
    for rule in ('yield to everybody', 'give_way(entry)'):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap)
        if rule != 'yield to everybody':
            sim.give_way('entry')
        ctx.synchronize()
        t0 = time.perf_counter()
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        ep = sim.episodes()
        seen = np.isfinite(ep['min_clearance'])
        cols[rule] = ('%d' % taken, '%d of %d' % (len(ep), total), '%.1f s' % (float(ep['delay'].mean()) * sim.params.dt if len(ep) else float('nan')),
                      '%d' % int(ep['contact'].sum()), '%.2f m' % (float(ep['min_clearance'][seen].min()) if seen.any() else float('inf')),
                      '%d' % (sim.active_count() + sim.waiting_count()), '%.2f s' % wall)
    names = list(cols)
    print('%-28s %22s %22s' % ('', names[0], names[1]))
    for i, what in enumerate(('steps taken', 'vehicles served', 'mean delay', 'contacts', 'worst clearance', 'still driving or waiting', 'wall time')):
        print('%-28s %22s %22s' % (what, cols[names[0]][i], cols[names[1]][i]))


if __name__ == '__main__':
    main()
