#!/usr/bin/env python3
"""What car following does to the flows whose outcome is contacts and worst clearance.

The open intersection and the demand of examples/reserved_flow.py -- the eight stock routes as eight slots, two per approach arm, every arm
one queue fed by a seeded memoryless arrival stream at a SHORT mean headway -- in three scenes, each run without and with
IntersectionBatch.follow() on the same demand:

    reservations, strict      reserve(dict(detect, patience=0)): strict first come, first served
    reservations, first fit   reserve(dict(detect, patience=None)): a denied request never blocks a later one
    plan + give_way           the fixed plan batch.two_phase_plan(cycle, green, amber) with give_way('entry'): queues behind the stop lines

Printed side by side: steps taken, vehicles served (arrivals), mean queueing delay, contacts and worst clearance (true clearance, from the
run log's outcome words), and with following the agents that had a leader in the last step.

    python examples/following_flow.py [--instances 64] [--headway 8] [--vehicles 4] [--gap 2.0] [--max-steps 1200] [--chunk 32]
                                      [--horizon 13] [--seed 0] [--cycle 100] [--green 30] [--amber 8] [--detect 100]
                                      [--standstill 6.0] [--time-gap 1.0] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SCENES = ('reservations, strict', 'reservations, first fit', 'plan + give_way')


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
    ap.add_argument('--standstill', type=float, default=6.0, help='following: distance kept to a leader at rest [m]')
    ap.add_argument('--time-gap', type=float, default=1.0, help='following: plus this many seconds of the follower\'s own speed')
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
          'fixed plan: cycle %d, green %d, amber %d; reservations: detector %d points; following: standstill %.1f m, time gap %.1f s'
          % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps, args.cycle, args.green, args.amber, args.detect,
             args.standstill, args.time_gap))
    cols = {}
    for scene in SCENES:
        for follow in (False, True):
            sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
            due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
            sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
            sim.retire_at_goal(leave_scene=True)
            sim.respawn_on_schedule(due, gap=args.gap)
            if scene == 'plan + give_way':
                sim.give_way('entry')
                sim.signalise(two_phase_plan(args.cycle, args.green, args.amber))
            else:
                sim.reserve(dict(detect=args.detect, patience=0 if scene.endswith('strict') else None))
            if follow:
                sim.follow(standstill=args.standstill, time_gap=args.time_gap)
            ctx.synchronize()
            t0 = time.perf_counter()
            taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
            ctx.synchronize()
            wall = time.perf_counter() - t0
            sim.check()
            ep = sim.episodes()
            seen = np.isfinite(ep['min_clearance'])
            cols[scene, follow] = ('%d' % taken, '%d of %d' % (len(ep), total),
                                   '%.1f s' % (float(ep['delay'].mean()) * sim.params.dt if len(ep) else float('nan')),
                                   '%d' % int(ep['contact'].sum()), '%.2f m' % (float(ep['min_clearance'][seen].min()) if seen.any() else float('inf')),
                                   '%d' % (sim.active_count() + sim.waiting_count()),
                                   '%d' % int((sim.leader >= 0).sum().item()) if follow else '-', '%.2f s' % wall)
    for scene in SCENES:
        print('\n%-28s %20s %20s' % (scene, 'without following', 'with following'))
        for i, what in enumerate(('steps taken', 'vehicles served', 'mean delay', 'contacts', 'worst clearance', 'still driving or waiting',
                                  'with a leader at the end', 'wall time')):
            print('%-28s %20s %20s' % (what, cols[scene, False][i], cols[scene, True][i]))


if __name__ == '__main__':
    main()
