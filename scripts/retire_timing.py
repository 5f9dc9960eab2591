#!/usr/bin/env python3
"""What retirement at the goal (IntersectionBatch.retire_at_goal) does to the time of an episode, and whether parked agents are the slow
problems of a QP launch.  Workloads: the stock family (A = 1, K = 2) at 1024 and 4096 instances, run to the last arrival (the number of
steps the retired run needs, rounded up to the chunk; the unretired run takes the same number), and 512 x 8 coupled agents for a fixed 200
steps.  Each workload without and with retirement in one process after a warm-up run, `--reps` repetitions each, timed with HIP events
around the whole run; reported: median and range per episode, the mean QP launch time (mpcx_profile_qp, one extra pass) before and
after the first arrival, and the maximum iteration count per step (closed_loop_stats, step by step, one extra pass).

    python scripts/retire_timing.py [--reps 5] [--horizon 20] [--only NAME]
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
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--max-steps', type=int, default=400)
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    T = args.horizon
    work = {'stock_1024': lambda: scripted_traffic_batch(ctx, B=1024, T=T, seed=0, A=1, K=2, routes=routes, dl=dl, cd=cd),
            'stock_4096': lambda: scripted_traffic_batch(ctx, B=4096, T=T, seed=0, A=1, K=2, routes=routes, dl=dl, cd=cd),
            'coupled_512x8': lambda: synthetic_batch(ctx, B=512, A=8, T=T, seed=0, routes=routes, dl=dl, cd=cd)}
    for name, make in work.items():
        if args.only and args.only != name:
            continue
        # the length of the episode: to the last arrival for the stock family, 200 steps for the coupled agents
        if name.startswith('coupled'):
            steps = 200
        else:
            probe = make()
            probe.retire_at_goal()
            steps = probe.run_until_done(args.max_steps, chunk=16)
            print('%s: last arrival within %d steps, %d egos still driving' % (name, steps, probe.active_count()), flush=True)
        res = {'workload': name, 'steps': steps, 'T': T}
        for retire in (False, True):
            tag = 'retire' if retire else 'plain'

            def fresh():
                sim = make()
                if retire:
                    sim.retire_at_goal()
                return sim
            fresh().run(steps)              # warm-up
            ctx.synchronize()
            ms = []
            for _ in range(args.reps):
                sim = fresh()
                ctx.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sim.run(steps)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            res[tag + '_ms'] = [round(m, 3) for m in ms]
            # one more pass, step by step: QP launch time and the step's maximum iteration count, before / after the first arrival
            sim = fresh()
            log = sim.attach_log(0)
            ctx.profile_qp(True)
            qp, mx, arrived = [], [], []
            ctx.closed_loop_stats(reset=True)
            for _ in range(steps):
                sim.run(1)
                t, n = ctx.profile_qp_read()
                qp.append(t / max(n, 1))
                mx.append(ctx.closed_loop_stats(reset=True)['max_iterations'])
                arrived.append(int((log.goal_step >= 0).sum().item()))
            ctx.profile_qp(False)
            qp, mx, arrived = np.array(qp), np.array(mx), np.array(arrived)
            first = int(np.argmax(arrived > 0)) if (arrived > 0).any() else steps
            res[tag + '_qp_ms_before_first_arrival'] = round(float(qp[1:first].mean()), 4) if first > 1 else None
            res[tag + '_qp_ms_after_first_arrival'] = round(float(qp[first:].mean()), 4) if first < steps else None
            res[tag + '_max_iters_before'] = int(mx[:first].max()) if first else None
            res[tag + '_max_iters_after'] = int(mx[first:].max()) if first < steps else None
            res[tag + '_mean_of_step_max_iters_before'] = round(float(mx[:first].mean()), 2) if first else None
            res[tag + '_mean_of_step_max_iters_after'] = round(float(mx[first:].mean()), 2) if first < steps else None
            res['first_arrival_step'] = first + 1
            res[tag + '_arrived'] = int(arrived[-1])
        for tag in ('plain', 'retire'):
            m = np.array(res[tag + '_ms'])
            res[tag + '_median_ms'], res[tag + '_min_ms'], res[tag + '_max_ms'] = round(float(np.median(m)), 3), float(m.min()), float(m.max())
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
