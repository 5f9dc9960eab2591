#!/usr/bin/env python3
"""What a speed advised ahead of a red light does to a signalised crossing in speed mode.

The straight scene -- the four straight stock routes, one car each from the first point of its route -- as a seeded family: every instance
starts its signal clock at a seeded point of the two-phase plan.  In speed mode (stop_mode='speed') a red light zeroes the speed reference
from the stop line on while the path stays whole, so a car reaches its line at speed, brakes late and creeps over: cars of both phases
meet inside the crossing.  The family is run twice, under IntersectionBatch.signalise() alone and with IntersectionBatch.advise_speed(),
which caps the speed reference of a car that would arrive on red at the speed with which it arrives as the light turns green.  Printed
side by side, from the run log: arrivals, steps with cars of both phases inside the crossing square, contacts and worst clearance.

    python examples/advised_flow.py [--instances 64] [--max-steps 400] [--chunk 16] [--horizon 13] [--seed 0] [--cycle 100] [--green 30]
                                    [--amber 8] [--v-min 1.0] [--lead 1] [--reach 60] [--graph]
"""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HALF_WIDTH = 12.0       # the stock crossing: a square of this half width about the origin
STRAIGHT = (1, 3, 5, 7)


def family(ctx, routes, dl, cd, B, T):
    """B instances x 4 agents in speed mode: agent a on the straight route of arm a + 1, from its first point"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.lib import mpc_with_speed
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams
    route = np.tile(np.array(STRAIGHT), (B, 1))
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    params = dataclasses.replace(mpc_with_speed.params(cd, 0.2), T=T, L=cd.distance_back_to_front_wheel)
    return IntersectionBatch(ctx, params, ip, routes, dl, route, np.zeros_like(route), stop_mode='speed')


def mixed_steps(log, B):
    """per instance, the steps after which cars of both phases (arms 1 / 3 and arms 2 / 4) were inside the crossing square"""
    rows, steps = log.rows(), log.outcomes()['steps']
    live = np.arange(rows.shape[0])[:, None] < steps[None, :]           # a retired agent has no row after its arrival
    inside = (live & (np.maximum(np.abs(rows['x']), np.abs(rows['y'])) <= HALF_WIDTH)).reshape(rows.shape[0], B, 4)
    return (inside[:, :, [0, 2]].any(axis=2) & inside[:, :, [1, 3]].any(axis=2)).sum(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=64)
    ap.add_argument('--max-steps', type=int, default=400)
    ap.add_argument('--chunk', type=int, default=16)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--cycle', type=int, default=100, help='signal cycle in steps')
    ap.add_argument('--green', type=int, default=30, help='green of each of the two phases in steps')
    ap.add_argument('--amber', type=int, default=8, help='amber after each green in steps')
    ap.add_argument('--v-min', type=float, default=1.0, help='the advised speed is never below this [m/s]')
    ap.add_argument('--lead', type=int, default=1, help='steps of margin after the light turns green')
    ap.add_argument('--reach', type=float, default=60.0, help='cars within this distance of their line are advised [m]')
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import stock_routes, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    plan = two_phase_plan(args.cycle, args.green, args.amber)
    offset = np.random.default_rng(args.seed).integers(0, args.cycle, args.instances)
    print('%d instances x 4 straight routes, speed mode, T = %d, plan: cycle %d, green %d, amber %d; clocks seeded (%d); at most %d steps'
          % (args.instances, args.horizon, args.cycle, args.green, args.amber, args.seed, args.max_steps))
    cols = {}
    for rule in ('signals', 'signals + advice'):
        sim = family(ctx, routes, dl, cd, args.instances, args.horizon)
        log = sim.attach_log(args.max_steps + args.chunk)
        sim.retire_at_goal(leave_scene=True)
        sim.signalise(plan, offset=offset)
        if rule != 'signals':
            sim.advise_speed(v_min=args.v_min, lead=args.lead, reach=args.reach)
        ctx.synchronize()
        t0 = time.perf_counter()
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        out = log.outcomes()
        there = out['goal_step'] >= 0
        mixed = mixed_steps(log, args.instances)
        seen = np.isfinite(out['min_clearance'])
        cols[rule] = ('%d' % taken, '%d of %d' % (int(there.sum()), sim.P),
                      '%.1f / %d' % (float(out['goal_step'][there].mean()) if there.any() else float('nan'), int(out['goal_step'].max())),
                      '%d of %d' % (int((mixed > 0).sum()), args.instances), '%.1f / %d' % (float(mixed.mean()), int(mixed.max())),
                      '%d' % int((out['contact_step'] >= 0).sum()), '%.2f m' % (float(out['min_clearance'][seen].min()) if seen.any() else float('inf')),
                      '%.2f s' % wall)
    names = list(cols)
    print('%-44s %20s %20s' % ('', names[0], names[1]))
    for i, what in enumerate(('steps taken', 'cars arrived', 'arrival step, mean / last', 'instances with both phases in the square',
                              'such steps per instance, mean / most', 'cars with a contact', 'worst clearance', 'wall time')):
        print('%-44s %20s %20s' % (what, cols[names[0]][i], cols[names[1]][i]))


if __name__ == '__main__':
    main()
