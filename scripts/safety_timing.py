#!/usr/bin/env python3
"""What the near-miss log costs at the headline batch: bench.py's flagship workload (synthetic_batch, instances x 8 agents on the stock
routes, T = 20, seed 1000).

  * per launch: the batch is driven `--steps` steps with watch_safety() on, so that the buffers and the context's prediction hold a real
    step; then mpcx_safety_step_batch is launched `--launches` times back to back on those buffers between a pair of HIP events (its
    decisions do not depend on its own words: every launch does the same searches; the ticks run on).  Beside it, as the yardstick, the
    conflict search's stage entry (mpcx_interaction_batch: prediction + search, two launches) the same way.  Back-to-back launches of one
    kernel overlap their launch overheads: the figure is the kernel's own time on an otherwise idle device.
  * per step: `--steps` steps of run() with the stage off and on, alternated, `--reps` times each: median and range of the time per step.

    python scripts/safety_timing.py [--reps 5] [--launches 200] [--instances 4096] [--agents 8] [--horizon 20] [--steps 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--agents', type=int, default=8)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--steps', type=int, default=30)
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    res = {'workload': 'synthetic_batch, %d x %d agents, T = %d, seed 1000' % (args.instances, args.agents, args.horizon),
           'launches': args.launches, 'steps': args.steps}
    fresh = lambda: synthetic_batch(ctx, B=args.instances, A=args.agents, T=args.horizon, seed=1000, routes=routes, dl=dl, cd=cd)

    # ---- per launch
    sim = fresh()
    sim.watch_safety()
    sim.run(args.steps)
    ctx.synchronize()
    s = sim._safety

    def safety():
        ctx.safety_step(sim.ip, sim.state, sim.path_off, sim.traj_idx, sim.obs6, sim.obs_off, sim.obs_cnt, sim.obs_skip, s)

    def search():
        ctx.interaction(sim.ip, sim.state, sim.path, sim.path_cs, sim.path_off, sim.path_len, sim.inter['cut_len'], sim.obs6, sim.obs_off,
                        sim.obs_cnt, sim.obs_skip, sim.traj_idx, out=sim.inter)
    for name, fn in (('safety_kernel', safety), ('prediction_and_conflict_search', search)):
        fn()
        ctx.synchronize()
        us = []
        stream = torch.cuda.current_stream(ctx.device)
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.launches):
                fn()
            e1.record(stream)
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / args.launches)
        res[name + '_us_per_launch'] = [round(float(v), 2) for v in us]
        res[name + '_median_us'] = round(float(np.median(us)), 2)
    res['with_a_partner'] = int((sim.partner >= 0).sum().item())
    res['with_a_predicted_contact'] = int((sim.ttc_frame >= 0).sum().item())
    res['events'] = int(sim.n_events.sum().item())
    del sim

    # ---- per step, off against on
    per = {'off': [], 'on': []}
    for _ in range(args.reps):
        for which in ('off', 'on'):
            sim = fresh()
            if which == 'on':
                sim.watch_safety()
            sim.run(5)
            ctx.synchronize()
            t0 = time.perf_counter()
            sim.run(args.steps)
            ctx.synchronize()
            per[which].append(1e6 * (time.perf_counter() - t0) / args.steps)
            del sim
    for which, us in per.items():
        res['step_%s_us' % which] = [round(v, 1) for v in us]
        res['step_%s_median_us' % which] = round(float(np.median(us)), 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
