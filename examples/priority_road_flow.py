#!/usr/bin/env python3
"""What a priority road does to the open intersection.

The flow of examples/open_intersection_flow.py on the same seeds -- the eight stock routes as eight slots, two per approach arm, every arm
one queue fed by a seeded memoryless arrival stream, following on -- as a junction without lights: arms 1 and 3 are the major road, arms 2
and 4 the minor road under give-way signs.  Run twice: with all roads equal (the conflict search alone sorts the cars out, whoever is
there first goes) and with IntersectionBatch.priority_road(): a minor-road car, or a major-road car turning across the opposed stream, waits
at its line until the conflicting movements of smaller rank leave it its critical gap.

Both runs carry the stage, the first with gap = 0: it then holds nobody and changes no byte of the run, and still writes every agent's lag,
so the lags the drivers ACCEPTED -- the last lag an agent had before it passed its line -- are measured the same way in both.

Printed side by side: steps taken, vehicles served and mean queueing delay per road (from the episode table), contacts and worst clearance
(from the run log's outcome words), the agent-steps spent yielding, and the share of accepted lags below the critical gap.

    python examples/priority_road_flow.py [--instances 64] [--headway 25] [--vehicles 3] [--gap 2.0] [--critical-gap 4.0] [--max-steps 600]
                                          [--horizon 13] [--seed 0] [--standstill 6.0] [--time-gap 1.0] [--graph]
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
    ap.add_argument('--headway', type=float, default=25.0, help='mean headway of an approach queue in steps (>= 1)')
    ap.add_argument('--vehicles', type=int, default=3, help='vehicles per slot (two slots per approach arm)')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a vehicle needs at its start pose to be let in')
    ap.add_argument('--critical-gap', type=float, default=4.0, help='seconds a yielding movement needs to the next conflicting car of smaller rank')
    ap.add_argument('--max-steps', type=int, default=600)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--standstill', type=float, default=6.0, help='following: distance kept to a leader at rest [m]')
    ap.add_argument('--time-gap', type=float, default=1.0, help='following: plus this many seconds of the follower\'s own speed')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    total = args.instances * 8 * args.vehicles
    print('%d instances x 8 slots x %d vehicles = %d, mean headway %.1f steps, gap %.1f m, seed %d, at most %d steps; major road: arms 1 and 3, '
          'critical gap %.1f s; following: standstill %.1f m, time gap %.1f s'
          % (args.instances, args.vehicles, total, args.headway, args.gap, args.seed, args.max_steps, args.critical_gap, args.standstill, args.time_gap))
    cols = {}
    for rule in (False, True):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.attach_log(0)               # outcomes only: contact and worst clearance per episode
        sim.retire_at_goal(leave_scene=True)
        sim.respawn_on_schedule(due, gap=args.gap)
        sim.priority_road(gap=args.critical_gap if rule else 0.0)       # (gap = 0: the stage measures and holds nobody)
        sim.follow(standstill=args.standstill, time_gap=args.time_gap)
        stop = sim._priority_tabs['path_stop']
        ctx.synchronize()
        t0 = time.perf_counter()
        taken, yielding, accepted = 0, 0, []
        for _ in range(args.max_steps):     # step by step: the lag is a last-step word
            ti0, off0, lag0, live0 = sim.traj_idx.clone(), sim.path_off.clone(), sim.lag.clone(), sim.done == 0
            if sim.run_until_done(1, chunk=1, graph=args.graph) < 1:
                break
            taken += 1
            yielding += int(sim.n_yielding.sum().item())
            line = stop[(off0 + ti0).long()]
            passed = live0 & (line >= 0) & (ti0 < line) & (sim.traj_idx >= line) & (sim.path_off == off0) & torch.isfinite(lag0)
            accepted.append(lag0[passed].cpu().numpy())
            if sim.active_count() + sim.waiting_count() == 0:
                break
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        ep = sim.episodes()
        minor = (ep['slot'] % 8 // 2) % 2 == 1          # slots 2k and 2k + 1 serve arm k + 1: arms 2 and 4 are the minor road
        seen = np.isfinite(ep['min_clearance'])
        acc = np.concatenate(accepted) if accepted else np.zeros(0)
        mean = lambda v: '%.1f s' % (float(v.mean()) * sim.params.dt) if len(v) else 'n/a'
        cols[rule] = ('%d' % taken, '%d of %d' % (len(ep), total), '%d / %d' % (int((~minor).sum()), int(minor.sum())),
                      '%s / %s' % (mean(ep['delay'][~minor]), mean(ep['delay'][minor])), '%d' % int(ep['contact'].sum()),
                      '%.2f m' % (float(ep['min_clearance'][seen].min()) if seen.any() else float('inf')),
                      '%d' % (sim.active_count() + sim.waiting_count()), '%d' % yielding,
                      '%d of %d (%.1f %%)' % (int((acc < args.critical_gap).sum()), len(acc), 100.0 * float((acc < args.critical_gap).mean()) if len(acc) else 0.0),
                      '%.2f s' % wall)
    print('\n%-40s %24s %24s' % ('', 'all roads equal', 'priority road'))
    for i, what in enumerate(('steps taken', 'vehicles served', '... major / minor road', 'mean delay, major / minor road', 'contacts', 'worst clearance',
                              'still driving or waiting', 'agent-steps yielding', 'accepted lags below the critical gap', 'wall time')):
        print('%-40s %24s %24s' % (what, cols[False][i], cols[True][i]))


if __name__ == '__main__':
    main()
