#!/usr/bin/env python3
"""What the two firm-hold kernels cost per launch at the headline batch: bench.py's flagship workload (synthetic_batch, instances x 8 agents
on the stock routes, T = 20, seed 1000) in speed mode under signalise(two_phase_plan(...)) is driven `--steps` steps with hold_firmly() on,
so that the buffers hold a real step; then each stage entry is launched `--launches` times back to back on those buffers between a pair of
HIP events -- mpcx_brake_mark_step_batch (a minimum on target_ind and plain words: launching it again changes nothing) and
mpcx_brake_clamp_step_batch on a scratch copy of traj_idx, overran and prev_len (a minimum on xref and on the index; overran counts, which
costs the same).  Reported: the median and range of the time per launch over `--reps` repetitions, in microseconds, and how many agents
were held firmly.  Back-to-back launches of one kernel overlap their launch overheads: the figure is the kernel's own time on an otherwise
idle device, not the cost of one more dependent launch in a step.

    python scripts/brake_timing.py [--reps 5] [--launches 200] [--instances 4096] [--agents 8] [--horizon 20] [--steps 30]
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
    ap.add_argument('--cycle', type=int, default=100)
    ap.add_argument('--green', type=int, default=30)
    ap.add_argument('--amber', type=int, default=8)
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import stock_routes, synthetic_batch, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0)
    routes, dl, cd = stock_routes(ctx)
    res = {'workload': 'synthetic_batch, %d x %d agents, T = %d, seed 1000, speed mode, two_phase_plan(%d, %d, %d), %d steps driven with hold_firmly()'
                       % (args.instances, args.agents, args.horizon, args.cycle, args.green, args.amber, args.steps), 'launches': args.launches}
    sim = synthetic_batch(ctx, B=args.instances, A=args.agents, T=args.horizon, seed=1000, routes=routes, dl=dl, cd=cd, stop_mode='speed')
    sim.signalise(two_phase_plan(args.cycle, args.green, args.amber))
    sim.hold_firmly()
    sim.run(args.steps)
    ctx.synchronize()
    br = sim._braking
    stop, held, boxed, yielding = sim._line_words()
    idx, seen, over = sim.traj_idx.clone(), sim.prev_len.clone(), sim.overran.clone()
    scratch = _lib.BrakingC(br.brake, br.setback, br.firm, over.data_ptr(), br.brake_cap)

    def mark():
        ctx.brake_mark_step(sim.dl, _lib.STOP_SPEED, sim.path_off, sim.path_len, sim.traj_idx, sim.target_ind, sim._win_len, stop, br, held=held,
                            boxed=boxed, yielding=yielding)

    def clamp():
        ctx.brake_clamp_step(sim.dl, sim.state, sim.path, sim.path_off, sim.path_len, idx, stop, scratch, sim.pre['xref'], prev_len=seen)
    for name, fn in (('brake_mark_kernel', mark), ('brake_clamp_kernel', clamp)):
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
        res['%s_us_per_launch' % name] = [round(float(v), 2) for v in us]
        res['%s_median_us' % name] = round(float(np.median(us)), 2)
    res['held_firmly'] = int((sim.firm != 0).sum().item())
    res['held'] = int((sim.held != 0).sum().item())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
