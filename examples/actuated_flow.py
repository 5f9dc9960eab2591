#!/usr/bin/env python3
"""What vehicle-actuated signals do to an intersection with unbalanced arms.

The open intersection of examples/signalised_flow.py -- the eight stock routes as eight slots, two per approach arm, every arm one queue fed
by a seeded memoryless arrival stream, every vehicle drawing its turning movement (batch.turning_demand) -- with a BUSY road (arms 1 and 3,
mean headway --headway) and a QUIET one (arms 2 and 4, --quiet-headway), run twice on the same seeds: under the fixed plan
batch.two_phase_plan(cycle, green, amber), which gives the quiet road its green whether anybody waits there or not, and under
batch.two_phase_controller(min_green, max_green, gap, amber, all_red, detect), the controller on the device that extends a green while cars
approach its lines and leaves it only for somebody who waits (IntersectionBatch.actuate).  Within a phase the cars settle their conflicts
first come, first served (give_way('entry')) unless --no-give-way is given.  Printed side by side: vehicles served, mean
queueing delay, contacts and worst clearance (true clearance, from the run log's outcome words).

    python examples/actuated_flow.py [--instances 64] [--headway 8] [--quiet-headway 60] [--vehicles 4] [--straight 0.7] [--gap 2.0]
                                     [--max-steps 1200] [--chunk 32] [--horizon 13] [--seed 0] [--cycle 100] [--green 30] [--amber 8]
                                     [--min-green 10] [--max-green 60] [--gap-out 5] [--detect 100] [--no-give-way]
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
    ap.add_argument('--headway', type=float, default=8.0, help='mean headway of the busy road\'s queues (arms 1 and 3) in steps (>= 1)')
    ap.add_argument('--quiet-headway', type=float, default=60.0, help='mean headway of the quiet road\'s queues (arms 2 and 4) in steps')
    ap.add_argument('--vehicles', type=int, default=4, help='vehicles per slot (two slots per approach arm)')
    ap.add_argument('--straight', type=float, default=0.7, help='share of the vehicles that go straight on')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a vehicle needs at its start pose to be let in')
    ap.add_argument('--max-steps', type=int, default=1200)
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--cycle', type=int, default=100, help='fixed plan: cycle in steps')
    ap.add_argument('--green', type=int, default=30, help='fixed plan: green of each of the two phases in steps')
    ap.add_argument('--amber', type=int, default=8, help='amber after each green in steps (both runs)')
    ap.add_argument('--min-green', type=int, default=10)
    ap.add_argument('--max-green', type=int, default=60)
    ap.add_argument('--gap-out', type=int, default=5, help='controller: steps without a call of its own after which a contested green ends')
    ap.add_argument('--detect', type=int, default=100, help='controller: length of the detector in front of a stop line in path points')
    ap.add_argument('--no-give-way', action='store_true', help='signals alone: within a phase everybody yields to everybody (default: first '
                    'come, first served, give_way(\'entry\'), the combination examples/signalised_flow.py finds best)')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, turning_demand, two_phase_controller, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    all_red = args.cycle // 2 - args.green - args.amber         # the plan's clearing gap; the controller gets the same
    sources = {'fixed plan': ('signalise', two_phase_plan(args.cycle, args.green, args.amber)),
               'actuated': ('actuate', two_phase_controller(args.min_green, args.max_green, args.gap_out, args.amber, all_red, args.detect))}
    total = args.instances * 8 * args.vehicles
    print('%s; ' % ('signals alone' if args.no_give_way else 'signals with first come, first served') +
          '%d instances x 8 slots x %d vehicles = %d; mean headway %.1f steps on arms 1 and 3, %.1f on arms 2 and 4; %.0f %% straight on; seed %d, '
          'at most %d steps\nfixed plan: cycle %d, green %d, amber %d, all-red %d; controller: min green %d, max green %d, gap %d, detector %d points'
          % (args.instances, args.vehicles, total, args.headway, args.quiet_headway, 100 * args.straight, args.seed, args.max_steps, args.cycle,
             args.green, args.amber, all_red, args.min_green, args.max_green, args.gap_out, args.detect))
    cols = {}
    for name, (method, arg) in sources.items():
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        zero = np.zeros_like(route)
        busy = demand_schedule(route, routes, zero, args.headway, args.vehicles, args.seed)
        quiet = demand_schedule(route, routes, zero, args.quiet_headway, args.vehicles, args.seed)
        due = np.where(((route // 2) % 2 == 0)[:, :, None], busy, quiet)            # (stock routes 2 k and 2 k + 1 leave arm k + 1)
        share = np.where(np.arange(len(routes)) % 2 == 1, args.straight, 1.0 - args.straight)     # (the odd stock routes go straight on)
        sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap, route=turning_demand(route, routes, zero, share, args.vehicles, args.seed))
        if not args.no_give_way:
            sim.give_way('entry')
        getattr(sim, method)(arg)
        ctx.synchronize()
        t0 = time.perf_counter()
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        ep = sim.episodes()
        seen = np.isfinite(ep['min_clearance'])
        cols[name] = ('%d' % taken, '%d of %d' % (len(ep), total), '%.1f s' % (float(ep['delay'].mean()) * sim.params.dt if len(ep) else float('nan')),
                      '%d' % int(ep['contact'].sum()), '%.2f m' % (float(ep['min_clearance'][seen].min()) if seen.any() else float('inf')),
                      '%d' % (sim.active_count() + sim.waiting_count()), '%.2f s' % wall)
    names = list(cols)
    print('%-28s %20s %20s' % ('', names[0], names[1]))
    for i, what in enumerate(('steps taken', 'vehicles served', 'mean delay', 'contacts', 'worst clearance', 'still driving or waiting', 'wall time')):
        print('%-28s %20s %20s' % (what, cols[names[0]][i], cols[names[1]][i]))


if __name__ == '__main__':
    main()
