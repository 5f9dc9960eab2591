#!/usr/bin/env python3
"""An OPEN intersection: cars arrive over time instead of all standing there at step 0.

A seeded family of instances x 8 agents on the eight stock routes, every one from the first point of its route.  The two routes of an
approach arm share that point, so every arm holds a queue of two cars.  batch.entry_schedule() draws memoryless headways per queue;
IntersectionBatch.enter_on_schedule() lets a car in, on the device, in the step it is due -- or the first later step in which its start pose
is `--gap` metres clear of everybody in the scene (the car ahead of it in its queue, as a rule).  Arrived cars leave the scene
(retire_at_goal(leave_scene=True)), and run_until_done() runs the whole episode in chunks without any host work between the steps.

    python examples/open_intersection_flow.py [--instances 256] [--headway 25] [--gap 2.0] [--max-steps 400] [--chunk 16] [--horizon 13]
                                              [--seed 0] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def family(ctx, routes, dl, cd, B, T):
    """B instances x 8 agents: agent a on stock route a, from its first point"""
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, MpcParams
    route = np.tile(np.arange(8), (B, 1))
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(ctx, MpcParams(T=T, L=cd.distance_back_to_front_wheel), ip, routes, dl, route, np.zeros_like(route)), route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=256)
    ap.add_argument('--headway', type=float, default=25.0, help='mean headway of an approach queue in steps (>= 1)')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a car needs at its start pose to be let in')
    ap.add_argument('--max-steps', type=int, default=400)
    ap.add_argument('--chunk', type=int, default=16, help='steps between two looks at the number of agents driving or waiting')
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import entry_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
    wait = entry_schedule(route, routes, np.zeros_like(route), args.headway, args.seed)
    log = sim.attach_log(0)                 # outcomes only: goal arrival, contact, worst clearance
    sim.retire_at_goal(leave_scene=True)
    sim.enter_on_schedule(wait, gap=args.gap)
    ctx.synchronize()
    t0 = time.perf_counter()
    taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    sim.check()
    out = log.outcomes()
    delay = sim.entry_delay()
    entered = delay >= 0
    held = delay > 0
    done = sim.done.cpu().numpy() != 0
    arrived = done & entered
    driven = sim.steps_driven.cpu().numpy()
    minc = out['min_clearance']
    seen = np.isfinite(minc)
    print('%d instances x 8 agents, mean headway %.1f steps, gap %.1f m: %d steps taken in %.3f s' % (args.instances, args.headway, args.gap, taken, wall))
    print('  entries %d of %d (still waiting %d); held by the gate %d, for %s steps (min / median / max)'
          % (int(entered.sum()), sim.P, sim.waiting_count(), int(held.sum()),
             '%d / %d / %d' % (delay[held].min(), np.median(delay[held]), delay[held].max()) if held.any() else '- / - / -'))
    print('  arrivals %d; steps per episode (min / median / max) %s; agents with a contact during their episode %d; worst clearance %.2f m'
          % (int(arrived.sum()), '%d / %d / %d' % (driven[arrived].min(), np.median(driven[arrived]), driven[arrived].max()) if arrived.any() else '- / - / -',
             int((out['contact_step'] >= 0).sum()), float(minc[seen].min()) if seen.any() else float('inf')))


if __name__ == '__main__':
    main()
