#!/usr/bin/env python3
"""What right of way costs per step: the open-intersection batch (examples/open_intersection_flow.py: instances x 8 agents on the eight stock
routes, all from the first point of their route) with the seeded demand of batch.demand_schedule() and every slot kept on its own route, in
three variants:

    routes    respawn_on_schedule(due, gap, route=): no precedence (mpcx_closed_loop_run_routes)
    equal     the same with give_way(order=<all zero>): the STAND / PREC instantiations of the prediction and the conflict search run, nobody
              yields in the rule's sense -- the run is the routes run bit for bit, so the difference is the rule's own cost
    entry     the same with give_way('entry'): one more dependent launch per step (the stamp), and traffic that flows differently

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step.  --parent TREE: the same `routes` workload also runs from another checkout of this project (the parent commit's tree,
built) as a child process within every repetition -- it has no precedence, so it runs scripts/route_timing.py's `routed` variant there.

    python scripts/precedence_timing.py [--reps 3] [--steps 150] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0] [--graph]
                                        [--parent TREE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

TAGS = ('routes', 'equal', 'entry')


def parent_run(tree, args):
    """one repetition of the parent tree's routed variant in a fresh child process; returns its median ms per step"""
    cmd = [sys.executable, os.path.join(tree, 'scripts', 'route_timing.py'), '--reps', '1', '--steps', str(args.steps), '--instances',
           str(args.instances), '--horizon', str(args.horizon), '--headway', str(args.headway), '--vehicles', str(args.vehicles), '--gap',
           str(args.gap), '--seed', str(args.seed), '--table-vehicles', '1', '--summary-reps', '1'] + (['--graph'] if args.graph else [])
    out = subprocess.run(cmd, cwd=tree, check=True, capture_output=True, text=True).stdout
    return float(json.loads(out.strip().splitlines()[-1])['routed_median_ms_per_step'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    ap.add_argument('--vehicles', type=int, default=3)
    ap.add_argument('--gap', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--parent', default=None, help='another checkout of this project (built) whose routed run is timed as a child process')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
        if tag == 'equal':
            sim.give_way(order=np.zeros_like(route))
        elif tag == 'entry':
            sim.give_way('entry')
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d%s'
                       % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, ', graph replay' if args.graph else ''),
           'steps': args.steps}
    for tag in TAGS:
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms, last, parent = {t: [] for t in TAGS}, {}, []
    for _ in range(args.reps):
        for tag in TAGS:
            sim = fresh(tag)
            ctx.synchronize()
            stream = torch.cuda.current_stream(ctx.device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sim.run(args.steps, args.graph)
            e1.record(stream)
            e1.synchronize()
            ctx.synchronize()
            ms[tag].append(e0.elapsed_time(e1) / args.steps)
            last[tag] = sim
        if args.parent:
            parent.append(parent_run(args.parent, args))
    for tag in TAGS:
        m, sim = np.array(ms[tag]), last[tag]
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_served'] = sim.served_count()
    if parent:
        res['parent_routed_ms_per_step'] = [round(v, 4) for v in parent]
        res['parent_routed_median_ms_per_step'] = round(float(np.median(parent)), 4)
    res['equal_minus_routes_ms_per_step'] = round(res['equal_median_ms_per_step'] - res['routes_median_ms_per_step'], 4)
    res['entry_minus_equal_ms_per_step'] = round(res['entry_median_ms_per_step'] - res['equal_median_ms_per_step'], 4)
    a, b = last['routes'], last['equal']
    res['equal_is_the_routes_run'] = bool(a.episodes().tobytes() == b.episodes().tobytes() and a.state.cpu().numpy().tobytes() == b.state.cpu().numpy().tobytes())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
