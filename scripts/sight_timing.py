#!/usr/bin/env python3
"""What line of sight costs on the open-intersection batch (examples/open_intersection_flow.py: instances x 8 agents on the stock routes from
their first points, T = 13, entered on a seeded schedule, retirement and departure on).

  * per step: four variants -- `plain` (no stage), `sight` with the empty set, `sight` with corner_blocks(), `sight` with the stock world's
    own 24 obstacles (medians and wrong-way lanes included: not a sensible occluder set, but the largest table the package serves for this
    world) -- alternated, `--reps` times each: a fresh batch, a warm-up of `--warmup` steps, then HIP events around run(`--steps`).
  * per stage call: the batch with corner_blocks() is driven `--warmup` steps so that the buffers hold a real step; then
    mpcx_sight_step_batch is called `--launches` times back to back between a pair of HIP events.  The figure is the time per CALL of the
    stage entry from Python -- the host's checks and enqueue or the kernel, whichever is longer -- and an upper bound of the kernel's time,
    not the kernel's time: for that take a kernel trace of this script (rocprofv3 --kernel-trace --stats, in a run of its own).

    python scripts/sight_timing.py [--reps 5] [--steps 100] [--warmup 20] [--launches 200] [--instances 256] [--horizon 13]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--instances', type=int, default=256)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import corner_blocks, entry_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.lib import scenario
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    world = list(scenario.intersection(1, 1).obstacles)
    sets = {'plain': None, 'sight_empty': [], 'sight_corner_blocks': corner_blocks(), 'sight_world_%d' % len(world): world}
    res = {'workload': 'open intersection, %d x 8 agents, T = %d' % (args.instances, args.horizon), 'steps': args.steps, 'warmup': args.warmup,
           'launches': args.launches}

    def fresh(occluders):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        sim.enter_on_schedule(entry_schedule(route, routes, np.zeros_like(route), args.headway, 0), gap=2.0)
        if occluders is not None:
            sim.occlude(occluders)
        return sim
    stream = torch.cuda.current_stream(ctx.device)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n

    # ---- per step, alternated
    per = {k: [] for k in sets}
    hidden = {}
    for _ in range(args.reps):
        for name, occ in sets.items():
            sim = fresh(occ)
            sim.run(args.warmup)
            ctx.synchronize()
            per[name].append(timed(lambda: sim.run(args.steps), args.steps))
            if occ is not None:
                hidden[name] = int(sim.n_hidden.sum().item())
            del sim
    for name, us in per.items():
        res['step_%s_us' % name] = [round(v, 1) for v in us]
        res['step_%s_median_us' % name] = round(float(np.median(us)), 1)
    res['hidden_rows_in_the_last_step'] = hidden

    # ---- per stage call
    sim = fresh(corner_blocks())
    sim.run(args.warmup)
    ctx.synchronize()

    def stage():
        for _ in range(args.launches):
            ctx.sight_step(sim.state, sim.obs6, sim.obs_off, sim.obs_cnt, sim.obs_skip, sim._sight, done=sim.done, absent=sim.absent)
    stage()
    ctx.synchronize()
    us = [timed(stage, args.launches) for _ in range(args.reps)]
    res['sight_stage_call_us'] = [round(v, 2) for v in us]
    res['sight_stage_call_median_us'] = round(float(np.median(us)), 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
