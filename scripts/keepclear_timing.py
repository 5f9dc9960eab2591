#!/usr/bin/env python3
"""What the keep-clear stage costs beside the signal stage it runs behind: the respawn batch of scripts/reserve_timing.py (instances x 8
agents on the eight stock routes, the seeded demand of batch.demand_schedule()) under a fixed two-phase plan in two variants:

    signals    signalise(two_phase_plan(...)): signal_kernel, a lane per agent
    keepclear  the same with keep_clear(): keepclear_kernel behind it, a lane group of 8 per junction -- one more launch per step

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run(steps); reported: median and
range of the time per step, and the stage's own cost per repetition against the run without it.  The stage changes what the cars do (boxed
cars wait), so the two runs do not solve the same QPs: --zero-table runs the stage with an all-zero conflict table, in which it launches,
classifies and writes its words but boxes nobody, and every other byte of the run is the plain run's -- the launch alone.
The kernels' own times (keepclear_kernel beside signal_kernel) come from a run of its own under the profiler, which this script does not
start:

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/keepclear_timing.py --only keepclear --reps 1

    python scripts/keepclear_timing.py [--reps 3] [--steps 100] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0] [--graph]
                                       [--cycle 100] [--green 30] [--amber 8] [--zero-table] [--only TAG]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

TAGS = ('signals', 'keepclear')


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
    ap.add_argument('--cycle', type=int, default=100)
    ap.add_argument('--green', type=int, default=30)
    ap.add_argument('--amber', type=int, default=8)
    ap.add_argument('--zero-table', action='store_true', help='keep_clear(conflict=zeros): the launch alone, nobody is boxed')
    ap.add_argument('--only', choices=TAGS, default=None, help='run this variant alone (for a profiler run of its own)')
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    plan = two_phase_plan(args.cycle, args.green, args.amber)
    tags = TAGS if args.only is None else (args.only,)

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
        sim.signalise(plan)
        if tag == 'keepclear':
            sim.keep_clear(conflict=np.zeros(12, dtype=np.int32) if args.zero_table else None)
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d, plan %d / %d / %d%s%s'
                       % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, args.cycle, args.green, args.amber,
                          ', all-zero conflict table' if args.zero_table else '', ', graph replay' if args.graph else ''),
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
        res[tag + '_held_at_end'] = int((sim.held != 0).sum().item())
    if 'keepclear' in tags:
        sim = last['keepclear']
        res['keepclear_boxed_at_end'], res['keepclear_occupied_junctions_at_end'] = int(sim.boxed.sum().item()), int((sim.box_occupied != 0).sum().item())
    if args.only is None:           # the stage's own cost: per repetition against the run without it of the same repetition
        d = 1000.0 * (np.array(ms['keepclear']) - np.array(ms['signals']))
        res['keepclear_stage_us_per_step'] = [round(float(v), 2) for v in d]
        res['keepclear_stage_median_us_per_step'] = round(float(np.median(d)), 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
