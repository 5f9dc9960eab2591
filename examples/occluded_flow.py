#!/usr/bin/env python3
"""How many vehicles must be connected before the blind corner stops mattering: the open intersection of
examples/open_intersection_flow.py with a building on every corner.

The eight stock routes as eight agents per instance, entered by a seeded memoryless arrival stream, no signals, no right of way.
IntersectionBatch.occlude(corner_blocks()) puts the four corner buildings of the stock world between the arms: a car sees another only in
range and with no building across the line between their reference points -- unless the other car is CONNECTED: the cars that share their
plans (share_plans) also announce their pose, so they are seen round the corner, and on their plan.  The connected share is a batch
dimension: the instances are three slices of one batch with shares 0, 0.5 and 1 (every vehicle of a slice is connected with that
probability, seeded).  watch_safety() is on: the near-miss log reads the physical scene, so it sees the contacts that occlusion causes.
Printed per slice: arrivals, agents with a contact during their episode, worst clearance, encounters the log opened, and the hidden
agent-steps (candidates of a window that the agent did not see, summed over agents and steps).

    python examples/occluded_flow.py [--instances 96] [--headway 25] [--gap 2.0] [--max-steps 400] [--horizon 13] [--seed 0]
                                     [--range 60] [--setback 5] [--shrink 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHARES = (0.0, 0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=96, help='a multiple of 3: one third per connected share')
    ap.add_argument('--headway', type=float, default=25.0, help='mean headway of an approach queue in steps (>= 1)')
    ap.add_argument('--gap', type=float, default=2.0, help='clearance [m] a car needs at its start pose to be let in')
    ap.add_argument('--max-steps', type=int, default=400)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--range', type=float, default=60.0, help='sensor range [m]')
    ap.add_argument('--setback', type=float, default=5.0, help='the buildings\' inner corners stand at (+-setback, +-setback)')
    ap.add_argument('--shrink', type=float, default=0.0, help='taken off every side of every building [m]')
    args = ap.parse_args()
    if args.instances < 3 or args.instances % 3:
        ap.error('--instances must be a positive multiple of 3')

    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import corner_blocks, entry_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    B, per = args.instances, args.instances // 3
    sim, route = family(ctx, routes, dl, cd, B, args.horizon)
    # the same arrivals in every slice: the schedule of one slice, three times
    wait = np.tile(entry_schedule(route[:per], routes, np.zeros_like(route[:per]), args.headway, args.seed), (3, 1))
    rng = np.random.default_rng(args.seed)
    draw = rng.random((per, 8))
    share = np.concatenate([(draw < s).astype(np.int32) for s in SHARES]).reshape(-1)
    log = sim.attach_log(0)
    sim.retire_at_goal(leave_scene=True)
    sim.enter_on_schedule(wait, gap=args.gap)
    sim.share_plans(share=share)
    sim.occlude(corner_blocks(args.setback), sensor_range=args.range, shrink=args.shrink, hear='shared')
    sim.watch_safety()
    hidden = torch.zeros(sim.P, dtype=torch.int64, device=ctx.device)
    taken = 0
    for taken in range(1, args.max_steps + 1):
        sim.run(1)
        hidden += sim.n_hidden
        if taken % 16 == 0 and sim.waiting_count() == 0 and bool((sim.done != 0).all().item()):
            break
    sim.check()
    out = log.outcomes()
    done = (sim.done.cpu().numpy() != 0) & (sim.entry_delay() >= 0)
    hidden, events = hidden.cpu().numpy(), sim.n_events.cpu().numpy()
    print('%d instances x 8 agents in three slices, mean headway %.1f steps, buildings set back %.1f m, range %.0f m: %d steps'
          % (B, args.headway, args.setback, args.range, taken))
    print('  %-16s %9s %9s %16s %11s %19s' % ('connected share', 'arrivals', 'contacts', 'worst clearance', 'encounters', 'hidden agent-steps'))
    for k, s in enumerate(SHARES):
        sl = slice(k * per * 8, (k + 1) * per * 8)
        minc = out['min_clearance'][sl]
        seen = np.isfinite(minc)
        print('  %-16.2f %9d %9d %14.2f m %11d %19d' % (s, int(done[sl].sum()), int((out['contact_step'][sl] >= 0).sum()),
                                                       float(minc[seen].min()) if seen.any() else float('inf'), int(events[sl].sum()),
                                                       int(hidden[sl].sum())))


if __name__ == '__main__':
    main()
