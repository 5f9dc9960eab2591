#!/usr/bin/env python3
"""Who came close to whom: the near-miss log on the flows of examples/following_flow.py.

The open intersection and the demand of examples/following_flow.py -- the eight stock routes as eight slots, two per approach arm, every arm
one queue fed by a seeded memoryless arrival stream at a short mean headway -- under the fixed plan with give_way('entry') and under
first-fit reservations, each without and with IntersectionBatch.follow(), all with IntersectionBatch.watch_safety() on.  Printed per
flow: the run's own figures (steps, vehicles served, contacts and worst clearance from the run log's episode table), the number of
encounters the stage opened and stored, and the CONFLICT MATRIX summed over the instances: per pair (movement of the agent, movement of its
partner) the events, the events with a contact, the events with a predicted contact, the smallest clearance and the shortest time to a
predicted contact.  A movement is named arm>arm (1 = from the south, counter-clockwise as batch.stop_lines() numbers them).

    python examples/near_miss_flow.py [--instances 64] [--headway 8] [--vehicles 4] [--gap 2.0] [--max-steps 1200] [--chunk 32]
                                      [--horizon 13] [--seed 0] [--cycle 100] [--green 30] [--amber 8] [--detect 100]
                                      [--near 0.5] [--ttc 2.0] [--capacity 16] [--graph]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FLOWS = (('plan + give_way', False), ('plan + give_way', True), ('reservations, first fit', False), ('reservations, first fit', True))


def arm_of(x, y):
    """the arm a point far from the crossing lies on: 1 south, 2 west, 3 north, 4 east (batch.stop_lines()' groups plus one)"""
    return (1 if y < 0 else 3) if abs(y) >= abs(x) else (2 if x < 0 else 4)


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
    ap.add_argument('--near', type=float, default=0.5, help='an encounter is open while the clearance is below this [m]')
    ap.add_argument('--ttc', type=float, default=2.0, help='... or a contact is predicted within this many seconds')
    ap.add_argument('--capacity', type=int, default=16, help='events stored per slot')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    names = ['%d>%d' % (arm_of(*r[0, :2]), arm_of(*r[-1, :2])) for r in routes] + ['none']
    total = args.instances * 8 * args.vehicles
    print('%d instances x 8 slots x %d vehicles = %d, mean headway %.1f steps, gap %.1f m, seed %d, at most %d steps; near %.2f m, ttc %.1f s, '
          '%d events per slot' % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps, args.near, args.ttc,
                                  args.capacity))
    for scene, follow in FLOWS:
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.attach_log(0)
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap)
        if scene == 'plan + give_way':
            sim.give_way('entry')
            sim.signalise(two_phase_plan(args.cycle, args.green, args.amber))
        else:
            sim.reserve(dict(detect=args.detect, patience=None))
        if follow:
            sim.follow()
        sim.watch_safety(near=args.near, ttc=args.ttc, capacity=args.capacity)
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        sim.check()
        ep = sim.episodes()
        seen = np.isfinite(ep['min_clearance'])
        opened, ev = int(sim.n_events.sum().item()), sim.near_misses()
        print('\n%s%s: %d steps, %d of %d served, %d episodes with a contact, worst clearance %.2f m; %d encounters opened, %d stored'
              % (scene, ', with following' if follow else '', taken, len(ep), total, int(ep['contact'].sum()),
                 float(ep['min_clearance'][seen].min()) if seen.any() else float('inf'), opened, len(ev)))
        cm = sim.conflict_matrix()
        events, contacts, predicted = (cm[k].sum(axis=0) for k in ('events', 'contacts', 'predicted'))
        lo, ttc = cm['min_clearance'].min(axis=0), cm['min_ttc'].min(axis=0)
        print('  %-6s %-6s %8s %9s %10s %14s %9s' % ('agent', 'other', 'events', 'contacts', 'predicted', 'min clearance', 'min ttc'))
        for i, j in sorted(zip(*np.nonzero(events)), key=lambda c: (-contacts[c], -events[c])):
            print('  %-6s %-6s %8d %9d %10d %12.2f m %7.1f s' % (names[i], names[j], events[i, j], contacts[i, j], predicted[i, j], lo[i, j], ttc[i, j]))


if __name__ == '__main__':
    main()
