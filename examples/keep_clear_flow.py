#!/usr/bin/env python3
"""What keeping the crossing clear does to the signalised flow.

The flow of examples/following_flow.py's "plan + give_way" column with following on, on the same seeds -- the eight stock routes as eight
slots, two per approach arm, every arm one queue fed by a seeded memoryless arrival stream at a short mean headway, give_way('entry') --
under the fixed plan batch.two_phase_plan(cycle, green, amber) and under the controller batch.two_phase_controller(...), each run without and
with IntersectionBatch.keep_clear(): a car whose light lets it go waits at its line while a movement of the other phase that conflicts with
its own is inside the crossing.

Printed side by side: steps taken, vehicles served, mean queueing delay, contacts and worst clearance (from the run log's outcome words) and
the steps agents spent boxed; then, per run, the cells of the near-miss log's conflict matrix between movements of different phases.

    python examples/keep_clear_flow.py [--instances 64] [--headway 8] [--vehicles 4] [--gap 2.0] [--max-steps 1200] [--chunk 32]
                                       [--horizon 13] [--seed 0] [--cycle 100] [--green 30] [--amber 8] [--min-green 10] [--max-green 60]
                                       [--gap-out 5] [--detect 100] [--standstill 6.0] [--time-gap 1.0] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SCENES = ('fixed plan', 'actuated')


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
    ap.add_argument('--amber', type=int, default=8, help='amber after each green in steps (both scenes)')
    ap.add_argument('--min-green', type=int, default=10)
    ap.add_argument('--max-green', type=int, default=60)
    ap.add_argument('--gap-out', type=int, default=5, help='controller: steps without a call of its own after which a contested green ends')
    ap.add_argument('--detect', type=int, default=100, help='controller: length of the detector in front of a stop line in path points')
    ap.add_argument('--standstill', type=float, default=6.0, help='following: distance kept to a leader at rest [m]')
    ap.add_argument('--time-gap', type=float, default=1.0, help='following: plus this many seconds of the follower\'s own speed')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, two_phase_controller, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    arm_of = lambda x, y: (1 if y < 0 else 3) if abs(y) >= abs(x) else (2 if x < 0 else 4)
    arms = [arm_of(*r[0, :2]) for r in routes]
    names = ['%d>%d' % (arm_of(*r[0, :2]), arm_of(*r[-1, :2])) for r in routes]
    total = args.instances * 8 * args.vehicles
    all_red = args.cycle // 2 - args.green - args.amber
    print('%d instances x 8 slots x %d vehicles = %d, mean headway %.1f steps, gap %.1f m, seed %d, at most %d steps\n'
          'fixed plan: cycle %d, green %d, amber %d (all-red %d); controller: min green %d, max green %d, gap-out %d, detector %d points; '
          'following: standstill %.1f m, time gap %.1f s'
          % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps, args.cycle, args.green, args.amber, all_red,
             args.min_green, args.max_green, args.gap_out, args.detect, args.standstill, args.time_gap))
    cols, cells = {}, {}
    for scene in SCENES:
        for keep in (False, True):
            sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
            due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
            sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
            sim.retire_at_goal(leave_scene=True)
            sim.respawn_on_schedule(due, gap=args.gap)
            sim.give_way('entry')
            if scene == 'fixed plan':
                sim.signalise(two_phase_plan(args.cycle, args.green, args.amber))
            else:
                sim.actuate(two_phase_controller(args.min_green, args.max_green, args.gap_out, args.amber, all_red, args.detect))
            if keep:
                sim.keep_clear()
            sim.follow(standstill=args.standstill, time_gap=args.time_gap)
            sim.watch_safety()
            ctx.synchronize()
            t0 = time.perf_counter()
            taken, boxed, left = 0, 0, args.max_steps
            while left > 0:                 # run_until_done in chunks of our own: the boxed words are last-step words, summed per step
                n = min(args.chunk, left) if not keep else 1
                got = sim.run_until_done(n, chunk=n, graph=args.graph)
                taken, left = taken + got, left - n
                if keep:
                    boxed += int(sim.n_boxed.sum().item())
                if got < n or sim.active_count() + sim.waiting_count() == 0:
                    break
            ctx.synchronize()
            wall = time.perf_counter() - t0
            sim.check()
            ep = sim.episodes()
            seen = np.isfinite(ep['min_clearance'])
            cols[scene, keep] = ('%d' % taken, '%d of %d' % (len(ep), total),
                                 '%.1f s' % (float(ep['delay'].mean()) * sim.params.dt if len(ep) else float('nan')),
                                 '%d' % int(ep['contact'].sum()), '%.2f m' % (float(ep['min_clearance'][seen].min()) if seen.any() else float('inf')),
                                 '%d' % (sim.active_count() + sim.waiting_count()), '%d' % boxed if keep else '-', '%.2f s' % wall)
            cm = sim.conflict_matrix()
            events, contacts = cm['events'].sum(axis=0), cm['contacts'].sum(axis=0)
            lo = cm['min_clearance'].min(axis=0)
            cells[scene, keep] = [(names[i], names[j], int(events[i, j]), int(contacts[i, j]), float(lo[i, j]))
                                  for i, j in sorted(zip(*np.nonzero(events[:8, :8])), key=lambda c: (-contacts[c], -events[c]))
                                  if (arms[i] - arms[j]) % 2 == 1]
    for scene in SCENES:
        print('\n%-28s %20s %20s' % (scene, 'enter on green', 'keep clear'))
        for i, what in enumerate(('steps taken', 'vehicles served', 'mean delay', 'contacts', 'worst clearance', 'still driving or waiting',
                                  'agent-steps boxed', 'wall time')):
            print('%-28s %20s %20s' % (what, cols[scene, False][i], cols[scene, True][i]))
    for scene in SCENES:
        for keep in (False, True):
            rows = cells[scene, keep]
            print('\n%s, %s: %d cross-phase cells of the conflict matrix, %d events, %d with a contact'
                  % (scene, 'keep clear' if keep else 'enter on green', len(rows), sum(r[2] for r in rows), sum(r[3] for r in rows)))
            print('  %-6s %-6s %8s %9s %14s' % ('agent', 'other', 'events', 'contacts', 'min clearance'))
            for r in rows:
                print('  %-6s %-6s %8d %9d %12.2f m' % r)


if __name__ == '__main__':
    main()
