#!/usr/bin/env python3
"""What the two following kernels cost per launch at the headline batch: bench.py's flagship workload (synthetic_batch, instances x 8
agents on the stock routes, T = 20, seed 1000) is driven `--steps` steps with follow() on, so that the buffers hold a real step; then each
stage entry is launched `--launches` times back to back on those buffers between a pair of HIP events -- mpcx_follow_step_batch (it only
lowers cut_len: launching it again changes nothing) and mpcx_follow_cap_step_batch (a minimum: the same).  Reported: the median and range
of the time per launch over `--reps` repetitions, in microseconds, how many agents had a leader, and the reach in points.  Back-to-back
launches of one kernel overlap their launch overheads: the figure is the kernel's own time on an otherwise idle device, not the cost of
one more dependent launch in a step.

    python scripts/follow_timing.py [--reps 5] [--launches 200] [--instances 4096] [--agents 8] [--horizon 20] [--steps 30] [--reach N]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument('--reach', type=int, default=None)
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    res = {'workload': 'synthetic_batch, %d x %d agents, T = %d, seed 1000, %d steps driven with follow()' % (args.instances, args.agents,
                                                                                                         args.horizon, args.steps),
           'launches': args.launches}
    for mode in ('cut', 'speed'):
        sim = synthetic_batch(ctx, B=args.instances, A=args.agents, T=args.horizon, seed=1000, routes=routes, dl=dl, cd=cd, stop_mode=mode)
        sim.follow(reach=args.reach)
        sim.run(args.steps)
        ctx.synchronize()
        fl = sim._following
        stop = _lib.STOP_SPEED if mode == 'speed' else _lib.STOP_CUT

        def search():
            ctx.follow_step(sim.dl, stop, sim.state, sim.path, sim.path_off, sim.path_len, sim.traj_idx, sim.inter['cut_len'], sim.obs6,
                            sim.obs_off, sim.obs_cnt, fl, obs_skip=sim.obs_skip)

        def clamp():
            ctx.follow_cap_step(fl, sim.pre['xref'])
        for name, fn in (('follow_kernel', search), ('follow_clamp_kernel', clamp)):
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
            us = np.array(us)
            res['%s_%s_us_per_launch' % (name, mode)] = [round(float(v), 2) for v in us]
            res['%s_%s_median_us' % (name, mode)] = round(float(np.median(us)), 2)
        res['with_a_leader_' + mode] = int((sim.leader >= 0).sum().item())
        res['capped_' + mode] = int((sim.follow_cap > 0).sum().item())
        res['reach_points'] = int(fl.reach)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
