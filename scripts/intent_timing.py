#!/usr/bin/env python3
"""What the shared-plans stage costs per step: the flagship workload (synthetic_batch: instances x 8 agents on the eight stock routes,
seeded starts, cut mode) in four variants:

    plain     no stage: step fusion applies (one launch for plant, prediction and rollout)
    idle      share_plans(all zero): intent_kernel runs between the prediction and the conflict search of every step and every wavefront
              leaves after its `frames` store -- the run is the unfused step bit for bit
    unfused   no stage, step fusion switched off: the launches of `idle` minus intent_kernel, so idle - unfused is the launch's own cost
    shared    share_plans(): every agent is seen on its plan (other traffic: other QPs)

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step and the differences.  shared - idle is the work of the kernel plus whatever the other traffic costs the QP.

    python scripts/intent_timing.py [--reps 5] [--steps 100] [--instances 4096] [--horizon 20] [--graph]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAGS = ('plain', 'unfused', 'idle', 'shared')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)

    def fresh(tag):
        sim = synthetic_batch(ctx, B=args.instances, A=8, T=args.horizon, seed=args.seed, routes=routes, dl=dl, cd=cd)
        if tag == 'idle':
            sim.share_plans(np.zeros(sim.P, np.int32))
        elif tag == 'shared':
            sim.share_plans()
        return sim

    def fusion(tag):
        ctx.set_step_fusion(tag == 'plain')
    res = {'workload': 'synthetic_batch, %d x 8 agents, T = %d, seed %d%s' % (args.instances, args.horizon, args.seed,
                                                                             ', graph replay' if args.graph else ''), 'steps': args.steps}
    for tag in TAGS:
        fusion(tag)
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms, last = {t: [] for t in TAGS}, {}
    for _ in range(args.reps):
        for tag in TAGS:
            fusion(tag)
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
    ctx.set_step_fusion(True)
    for tag in TAGS:
        m = np.array(ms[tag])
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        v = last[tag].state[:, 2]
        res[tag + '_mean_speed_at_end'] = round(float(v.mean().item()), 4)
        res[tag + '_standing_share_at_end'] = round(float((v.abs() <= 0.1389).double().mean().item()), 4)
        res[tag + '_mean_qp_iterations_at_end'] = round(float(last[tag].sol['iters'].double().mean().item()), 3)
    med = lambda t: res[t + '_median_ms_per_step']
    res['idle_minus_unfused_us_per_step'] = round(1e3 * (med('idle') - med('unfused')), 2)
    res['idle_minus_plain_us_per_step'] = round(1e3 * (med('idle') - med('plain')), 2)
    res['shared_minus_idle_us_per_step'] = round(1e3 * (med('shared') - med('idle')), 2)
    same = lambda a, b: bool(last[a].state.cpu().numpy().tobytes() == last[b].state.cpu().numpy().tobytes())
    res['idle_is_the_plain_run'] = same('idle', 'plain') and same('idle', 'unfused') and not last['idle'].shared_frames.any().item()
    res['agents_seen_on_plans_at_end'] = int((last['shared'].shared_frames > 0).sum().item())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
