#!/usr/bin/env python3
"""What the priority stage costs: the respawn batch of scripts/keepclear_timing.py (instances x 8 agents on the eight stock routes, the
seeded demand of batch.demand_schedule()) without lights in two variants:

    open      no hold at all: the conflict search alone
    priority  the same with priority_road(): priority_kernel in the hold's place, a lane group of 8 per junction, every lane meeting the
              seven others of its group -- one more launch per step

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run(steps); reported: median and
range of the time per step, and the stage's own cost per repetition against the run without it.  The stage changes what the cars do
(yielding cars wait), so the two runs do not solve the same QPs: --zero-gap runs the stage with gap = 0, in which it launches, classifies,
pairs every agent with every other and writes its words but holds nobody, and every other byte of the run is the plain run's -- the launch
alone.
The kernel's own time comes from a run of its own under the profiler, which this script does not start:

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/priority_timing.py --only priority --reps 1

    python scripts/priority_timing.py [--reps 3] [--steps 100] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0] [--graph]
                                      [--critical-gap 4.0] [--zero-gap] [--only TAG]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

TAGS = ('open', 'priority')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    ap.add_argument('--vehicles', type=int, default=3)
    ap.add_argument('--gap', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--critical-gap', type=float, default=4.0)
    ap.add_argument('--zero-gap', action='store_true', help='priority_road(gap=0): the launch alone, nobody yields')
    ap.add_argument('--only', choices=TAGS, default=None, help='run this variant alone (for a profiler run of its own)')
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    tags = TAGS if args.only is None else (args.only,)

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
        if tag == 'priority':
            sim.priority_road(gap=0.0 if args.zero_gap else args.critical_gap)
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d, critical gap %s%s'
                       % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, '0 (nobody yields)' if args.zero_gap else
                          '%.1f s' % args.critical_gap, ', graph replay' if args.graph else ''),
           'steps': args.steps}
    for tag in tags:
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms, last = {t: [] for t in tags}, {}
    stream = torch.cuda.current_stream(ctx.device)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ctx.synchronize()
        return e0.elapsed_time(e1) / n
    for _ in range(args.reps):
        for tag in tags:
            sim = fresh(tag)
            ctx.synchronize()
            ms[tag].append(timed(lambda: sim.run(args.steps, args.graph), args.steps))
            last[tag] = sim
    for tag in tags:
        m, sim = np.array(ms[tag]), last[tag]
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_served'] = sim.served_count()
    if 'priority' in tags:
        sim = last['priority']
        res['priority_yielding_at_end'], res['priority_occupied_junctions_at_end'] = int(sim.yielding.sum().item()), int((sim.crossing != 0).sum().item())
    if args.only is None:           # the stage's own cost: per repetition against the run without it of the same repetition
        d = 1000.0 * (np.array(ms['priority']) - np.array(ms['open']))
        res['priority_stage_us_per_step'] = [round(float(v), 2) for v in d]
        res['priority_stage_median_us_per_step'] = round(float(np.median(d)), 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
