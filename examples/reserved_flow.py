#!/usr/bin/env python3
"""What crossing reservations do to an intersection near capacity.

The open intersection and the demand of examples/right_of_way_flow.py -- the eight stock routes as eight slots, two per approach arm, every
arm one queue fed by a seeded memoryless arrival stream at a SHORT mean headway -- run three times on the same demand:

    give_way(entry)     first come, first served by order of entry, no signals (IntersectionBatch.give_way('entry'))
    plan + give_way     the fixed plan batch.two_phase_plan(cycle, green, amber) with give_way('entry') inside a phase
    reservations        IntersectionBatch.reserve(dict(detect, patience)): a manager per junction admits a car only if its movement
                        conflicts with no movement that holds the crossing; everybody else waits at its stop line

Printed side by side: vehicles served, mean queueing delay, contacts and worst clearance (true clearance, from the run log's outcome words,
in all columns).

    python examples/reserved_flow.py [--instances 64] [--headway 8] [--vehicles 4] [--gap 2.0] [--max-steps 1200] [--chunk 32]
                                     [--horizon 13] [--seed 0] [--cycle 100] [--green 30] [--amber 8] [--detect 100] [--patience 0]
                                     [--graph]
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
    ap.add_argument('--cycle', type=int, default=100, help='fixed plan: cycle in steps')
    ap.add_argument('--green', type=int, default=30, help='fixed plan: green of each of the two phases in steps')
    ap.add_argument('--amber', type=int, default=8, help='fixed plan: amber after each green in steps')
    ap.add_argument('--detect', type=int, default=100, help='reservations: a car requests the crossing from this many path points before its line')
    ap.add_argument('--patience', type=int, default=0, help='reservations: steps a denied request waits before it blocks every later request that '
                    'conflicts with it (0: strict first come, first served; negative: never)')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    total = args.instances * 8 * args.vehicles
    print('%d instances x 8 slots x %d vehicles = %d, mean headway %.1f steps, gap %.1f m, seed %d, at most %d steps\n'
          'fixed plan: cycle %d, green %d, amber %d; reservations: detector %d points, patience %s'
          % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps, args.cycle, args.green, args.amber, args.detect,
             'unbounded' if args.patience < 0 else '%d steps' % args.patience))
    cols = {}
    for rule in ('give_way(entry)', 'plan + give_way', 'reservations'):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap)
        if rule != 'reservations':
            sim.give_way('entry')
        if rule == 'plan + give_way':
            sim.signalise(two_phase_plan(args.cycle, args.green, args.amber))
        if rule == 'reservations':
            sim.reserve(dict(detect=args.detect, patience=None if args.patience < 0 else args.patience))
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
    print('%-28s' % '' + ''.join(' %20s' % n for n in names))
    for i, what in enumerate(('steps taken', 'vehicles served', 'mean delay', 'contacts', 'worst clearance', 'still driving or waiting', 'wall time')):
        print('%-28s' % what + ''.join(' %20s' % cols[n][i] for n in names))


if __name__ == '__main__':
    main()
