#!/usr/bin/env python3
"""Pairs of agents that SHARE AN EXIT ARM of the stock intersection, run as episodes twice: with retirement alone
(IntersectionBatch.retire_at_goal()) and with departure (retire_at_goal(leave_scene=True)).

Every exit arm is the goal of two of the eight stock routes -- (1,2)/(2,1), (2,2)/(3,1), (3,2)/(4,1), (4,2)/(1,1) end within a car's length
of each other.  With retirement alone the first agent to arrive parks there; the second one's conflict search finds the parked car and cuts
its path a car length short, mpc.is_goal can never hold and the episode never ends (and the log books a contact with a car whose episode the
reference's loop had already ended).  With departure the arrived car is taken out of everybody's obstacle list from the next step on.
A seeded family: instance b draws one of the four pairs and start offsets around the 10 m / 20 m case (the leader 8-12 m, the follower
17-27 m before the last point of its route), v0 = 0.

    python examples/shared_exit_episodes.py [--instances 256] [--max-steps 150] [--chunk 8] [--horizon 13] [--seed 0] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = ((1, 2), (3, 4), (5, 6), (7, 0))        # indices into stock_routes(): (1,2)/(2,1), (2,2)/(3,1), (3,2)/(4,1), (4,2)/(1,1)


def family(ctx, routes, dl, cd, B, T, seed):
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch
    from mpc_for_av_at_intersection_amd.runtime import InteractionParams, MpcParams
    rng = np.random.default_rng(seed)
    pair = np.array(PAIRS)[rng.integers(0, len(PAIRS), size=B)]
    back = np.column_stack([rng.uniform(8.0, 12.0, B), rng.uniform(17.0, 27.0, B)])
    lens = np.array([len(r) for r in routes])[pair]
    start = lens - 1 - np.rint(back / dl).astype(np.int64)
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    return IntersectionBatch(ctx, MpcParams(T=T, L=cd.distance_back_to_front_wheel), ip, routes, dl, pair, start)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=256)
    ap.add_argument('--max-steps', type=int, default=150)
    ap.add_argument('--chunk', type=int, default=8, help='steps between two looks at the number of agents still driving')
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    for leave in (False, True):
        sim = family(ctx, routes, dl, cd, args.instances, args.horizon, args.seed)
        log = sim.attach_log(0)                 # outcomes only: goal arrival, contact, worst clearance
        sim.retire_at_goal(leave_scene=leave)
        ctx.synchronize()
        t0 = time.perf_counter()
        taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        sim.check()
        out = log.outcomes()
        done = (sim.done.cpu().numpy() != 0).reshape(-1, 2)
        driven = sim.steps_driven.cpu().numpy().reshape(-1, 2)
        contact = (out['contact_step'] >= 0).reshape(-1, 2)
        minc = out['min_clearance'].reshape(-1, 2)
        seen = np.isfinite(minc)

        def ep(col):
            e = driven[done[:, col], col]
            return '%d / %d / %d' % (e.min(), np.median(e), e.max()) if len(e) else '- / - / -'
        print('%-22s %d instances x 2 agents, %d steps taken in %.3f s: leaders arrived %d, followers arrived %d of %d; steps per episode '
              '(min / median / max) leaders %s, followers %s; agents with a contact during their episode %d; worst clearance %.2f m'
              % ('leave_scene=True:' if leave else 'retirement alone:', args.instances, taken, wall, int(done[:, 0].sum()), int(done[:, 1].sum()),
                 args.instances, ep(0), ep(1), int(contact.sum()), float(minc[seen].min()) if seen.any() else float('inf')))


if __name__ == '__main__':
    main()
