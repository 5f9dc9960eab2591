#!/usr/bin/env python3
"""Step time of the open-intersection batch (examples/open_intersection_flow.py: instances x 8 agents on the eight stock routes, all from the
first point of their route) with admission against the same batch with retirement + departure only:

    depart      retire_at_goal(leave_scene=True) alone: everybody is in the scene from step 0 (the loop as it was before admission)
    admit_idle  the same with enter_on_schedule() and nobody scheduled: the same work plus the admission stage's two launches -- the
                stage's own cost
    admit       the seeded schedule of batch.entry_schedule(): agents enter over time (less work per step while they wait)

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step.  For the kernels' own times run one variant under the profiler:

    python scripts/admit_timing.py [--reps 5] [--steps 150] [--instances 4096] [--headway 25] [--gap 2.0] [--only depart|admit_idle|admit] [--graph]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/admit_timing.py --reps 1 --only admit_idle
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))

TAGS = ('depart', 'admit_idle', 'admit')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    ap.add_argument('--gap', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--only', default=None, choices=TAGS)
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import entry_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    tags = [t for t in TAGS if not args.only or args.only == t]

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        if tag == 'admit_idle':
            sim.enter_on_schedule(np.full(route.shape, -1))
        elif tag == 'admit':
            sim.enter_on_schedule(entry_schedule(route, routes, np.zeros_like(route), args.headway, args.seed), gap=args.gap)
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, gap %.1f, seed %d%s'
                       % (args.instances, args.horizon, args.headway, args.gap, args.seed, ', graph replay' if args.graph else ''), 'steps': args.steps}
    for tag in tags:
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms = {t: [] for t in tags}
    last = {}
    for _ in range(args.reps):
        for tag in tags:
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
    for tag in tags:
        m, sim = np.array(ms[tag]), last[tag]
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_arrived'] = int(((sim.done != 0) & (sim.steps_driven > 0)).sum().item())
        res[tag + '_waiting'] = sim.waiting_count()
    if 'depart' in ms and 'admit_idle' in ms:
        res['stage_overhead_ms_per_step'] = round(res['admit_idle_median_ms_per_step'] - res['depart_median_ms_per_step'], 4)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
