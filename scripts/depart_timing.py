#!/usr/bin/env python3
"""Step time of the benchmark workload (batch.synthetic_batch: 4096 instances x 8 agents, T = 20, seed 1000 as bench.py draws it) over 150
steps with retirement at the goal alone and with departure (retire_at_goal(leave_scene=True): arrived agents leave the scene).  Each variant
after a warm-up run, `--reps` repetitions, HIP events around the whole run; reported: median and range of the time per step, and how many
agents had arrived / left by the end.  For interaction_kernel's share of the kernel time run one variant under the profiler:

    python scripts/depart_timing.py [--reps 5] [--steps 150] [--instances 4096] [--only retire|depart]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/depart_timing.py --reps 1 --only depart
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--only', default=None, choices=['retire', 'depart'])
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    res = {'workload': 'synthetic_batch %d x 8, T = %d, seed %d' % (args.instances, args.horizon, args.seed), 'steps': args.steps}
    for tag in ('retire', 'depart'):
        if args.only and args.only != tag:
            continue

        def fresh():
            sim = synthetic_batch(ctx, B=args.instances, A=8, T=args.horizon, seed=args.seed, routes=routes, dl=dl, cd=cd)
            sim.retire_at_goal(leave_scene=(tag == 'depart'))
            return sim
        fresh().run(args.steps)             # warm-up
        ctx.synchronize()
        ms = []
        for _ in range(args.reps):
            sim = fresh()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sim.run(args.steps)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        m = np.array(ms)
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in ms]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_arrived'] = int((sim.done != 0).sum().item())
        if sim.absent is not None:
            res[tag + '_absent_rows'] = int((sim.absent != 0).sum().item())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
