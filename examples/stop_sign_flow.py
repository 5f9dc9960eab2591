#!/usr/bin/env python3
"""What stop signs do to the open intersection.

The flow of examples/open_intersection_flow.py on one seeded demand -- the eight stock routes as eight slots, two per approach arm, every
arm one queue fed by a seeded memoryless arrival stream, respawn with routes, following on -- as a junction without lights, run three ways:

    priority road   arms 1 and 3 are the major road, arms 2 and 4 give way (IntersectionBatch.priority_road())
    all-way stop    every arm carries a stop sign (IntersectionBatch.stop_signs())
    two-way stop    arms 2 and 4 carry stop signs, arms 1 and 3 are the through road (stop_signs(signed=(1, 3)))

in cut mode, and in speed mode with the firm hold (hold_firmly()).  Printed per way: vehicles served per arm, mean and worst queueing delay
per arm (from the episode table: what the gate and the slot's previous vehicle held a vehicle back for), contacts, the cars that entered a
signed movement without a release (ran_sign), and the total of the near-miss log's conflict matrix.

    python examples/stop_sign_flow.py [--instances 64] [--headway 25] [--vehicles 3] [--gap 2.0] [--critical-gap 5.0] [--max-steps 600]
                                      [--horizon 13] [--seed 0] [--standstill 6.0] [--time-gap 1.0] [--patience 0] [--modes cut,speed] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WAYS = ('priority road', 'all-way stop', 'two-way stop')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=64)
    ap.add_argument('--headway', type=float, default=25.0, help='mean headway of an approach queue in steps (>= 1)')
    ap.add_argument('--vehicles', type=int, default=3, help='vehicles per slot (two slots per approach arm)')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a vehicle needs at its start pose to be let in')
    ap.add_argument('--critical-gap', type=float, default=5.0, help='seconds a waiting movement needs to the next conflicting car of the through road')
    ap.add_argument('--max-steps', type=int, default=600)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--standstill', type=float, default=6.0, help='following: distance kept to a leader at rest [m]')
    ap.add_argument('--time-gap', type=float, default=1.0, help='following: plus this many seconds of the follower\'s own speed')
    ap.add_argument('--patience', type=int, default=0, help='stop signs: steps after which a denied car blocks the movements that cross its own')
    ap.add_argument('--modes', default='cut,speed', help='comma-separated: cut, speed (speed runs with the firm hold)')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from firm_hold_flow import speed_family
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    total = args.instances * 8 * args.vehicles
    print('%d instances x 8 slots x %d vehicles = %d, mean headway %.1f steps, gap %.1f m, seed %d, at most %d steps; critical gap %.1f s, patience %d '
          'steps; following: standstill %.1f m, time gap %.1f s'
          % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps, args.critical_gap, args.patience,
             args.standstill, args.time_gap))
    for mode in args.modes.split(','):
        cols = {}
        for way in WAYS:
            sim, route = (speed_family if mode == 'speed' else family)(ctx, routes, dl, cd, args.instances, args.horizon)
            due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
            sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
            sim.retire_at_goal(leave_scene=True)
            sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
            if way == 'priority road':
                sim.priority_road(gap=args.critical_gap)
            else:
                sim.stop_signs(signed=None if way == 'all-way stop' else (1, 3), gap=args.critical_gap, patience=args.patience)
            if mode == 'speed':
                sim.hold_firmly()
            sim.follow(standstill=args.standstill, time_gap=args.time_gap)
            sim.watch_safety()
            ctx.synchronize()
            t0 = time.perf_counter()
            taken = sim.run_until_done(args.max_steps, chunk=25, graph=args.graph)
            ctx.synchronize()
            wall = time.perf_counter() - t0
            sim.check()
            ep = sim.episodes()
            arm = ep['slot'] % 8 // 2
            dt = sim.params.dt
            per_arm = lambda f: ' / '.join(f(ep[arm == k]) for k in range(4))
            cm = sim.conflict_matrix()
            cols[way] = ('%d' % taken, '%d of %d' % (len(ep), total), per_arm(lambda e: '%d' % len(e)),
                         per_arm(lambda e: '%.1f' % (float(e['delay'].mean()) * dt) if len(e) else 'n/a'),
                         per_arm(lambda e: '%.1f' % (float(e['delay'].max()) * dt) if len(e) else 'n/a'),
                         '%d' % int(ep['contact'].sum()), 'n/a' if sim.ran_sign is None or way == 'priority road' else '%d' % int(sim.ran_sign.sum().item()),
                         '%d events, %d contacts' % (int(cm['events'].sum()), int(cm['contacts'].sum())),
                         '%d' % (sim.active_count() + sim.waiting_count()), '%.2f s' % wall)
        print('\n%-36s %30s %30s %30s' % ((mode + ' mode' + (', firm hold' if mode == 'speed' else ''),) + WAYS))
        for i, what in enumerate(('steps taken', 'vehicles served', '... per arm 1 / 2 / 3 / 4', 'mean queueing delay per arm [s]', 'worst queueing delay per arm [s]',
                                  'contacts', 'ran a sign', 'conflict matrix, total', 'still driving or waiting', 'wall time')):
            print('%-36s %30s %30s %30s' % ((what,) + tuple(cols[w][i] for w in WAYS)))


if __name__ == '__main__':
    main()
