#!/usr/bin/env python3
"""How does the crossing cope when more of the traffic turns?  The per-movement table of an open intersection at three turning shares.

Four approach arms with two SLOTS each; the two stock routes of an arm -- its two turning movements -- share their first point, so every arm
is one queue fed by one seeded memoryless arrival stream (batch.demand_schedule).  Every VEHICLE draws its own movement
(batch.turning_demand): `--shares` is the probability of the arm's second stock route, one batch per value.  When a vehicle arrives the slot
is reset, on the device, onto the next vehicle's route (IntersectionBatch.respawn_on_schedule(route=...)): the turning proportions vary
with no host work between the steps.  The table is reduced on the device too (movement_summary()): per route, over all instances, the
vehicles served, their mean queueing delay, their mean travel time and the episodes with a contact.

    python examples/intersection_turning_flow.py [--instances 64] [--shares 0.2,0.5,0.8] [--headway 30] [--vehicles 4] [--gap 2.0]
                                                 [--max-steps 2000] [--chunk 32] [--horizon 13] [--seed 0] [--graph]
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
    ap.add_argument('--shares', default='0.2,0.5,0.8', help='share of every arm\'s second stock route, comma-separated (each in [0, 1])')
    ap.add_argument('--headway', type=float, default=30.0, help='mean headway of an approach queue in steps (>= 1)')
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
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, turning_demand
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    print('%d instances x 4 arms x 2 slots x %d vehicles, mean headway %.1f steps, gap %.1f m, seed %d'
          % (args.instances, args.vehicles, args.headway, args.gap, args.seed))
    for share in (float(s) for s in args.shares.split(',')):
        sim, slot_route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        start = np.zeros_like(slot_route)
        due = demand_schedule(slot_route, routes, start, args.headway, args.vehicles, args.seed)
        route = turning_demand(slot_route, routes, start, [1.0 - share, share] * 4, args.vehicles, args.seed)
        sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap, route=route)
        ctx.synchronize()
        t0 = time.perf_counter()
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        tab = sim.movement_summary()            # (instances, 8 routes), reduced on the device
        n = tab['count'].sum(axis=0)
        print('share of the second movement %.2f: %d steps, %d of %d vehicles served (%.2f s wall)'
              % (share, taken, int(n.sum()), sim.P * args.vehicles, wall))
        print('%6s %8s %14s %14s %9s %10s' % ('route', 'served', 'mean delay', 'mean travel', 'contacts', 'clearance'))
        for r in range(len(routes)):
            k = max(int(n[r]), 1)
            print('%6d %8d %12.1f s %12.1f s %9d %8.2f m' % (r, n[r], tab['delay_sum'][:, r].sum() / k * sim.params.dt,
                                                            tab['steps_driven_sum'][:, r].sum() / k * sim.params.dt,
                                                            tab['contacts'][:, r].sum(), tab['min_clearance'][:, r].min()))


if __name__ == '__main__':
    main()
