#!/usr/bin/env python3
"""What respawn costs per step: the open-intersection batch (examples/open_intersection_flow.py: instances x 8 agents on the eight stock
routes, all from the first point of their route) with admission on in every variant:

    admit         retire_at_goal(leave_scene=True) + enter_on_schedule() with nobody scheduled: the loop as it was before respawn
    respawn_idle  the same words with the respawn stage switched on and nothing to do for it while the cars drive (a one-vehicle stream per
                  slot, nobody scheduled): the same work plus the stage's one launch -- the stage's own cost
    respawn       respawn_on_schedule() with the seeded demand of batch.demand_schedule(): vehicles enter, arrive and are replaced

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step.  The parent commit joins the alternation when --parent-tree names a checkout of it with its library built: once per
repetition a child process runs that tree's own scripts/admit_timing.py --only admit_idle, which is the `admit` variant here.

    python scripts/respawn_timing.py [--reps 5] [--steps 150] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0]
                                     [--only admit|respawn_idle|respawn] [--graph] [--parent-tree DIR]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/respawn_timing.py --reps 1 --only respawn_idle
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))

TAGS = ('admit', 'respawn_idle', 'respawn')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    ap.add_argument('--vehicles', type=int, default=3)
    ap.add_argument('--gap', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--only', default=None, choices=TAGS)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit: its admission-only run joins every repetition')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    tags = [t for t in TAGS if not args.only or args.only == t]

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        if tag == 'respawn':
            sim.respawn_on_schedule(demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed), gap=args.gap)
            return sim
        sim.enter_on_schedule(np.full(route.shape, -1))
        if tag == 'respawn_idle':       # everybody present from the start, as in `admit`; the stage on top, one vehicle per slot
            dev = ctx.device
            sim.start_state, sim.start_idx = sim.state.clone(), sim.traj_idx.clone()
            sim.due = torch.zeros((sim.P, 1), dtype=torch.int32, device=dev)
            sim.served = torch.zeros(sim.P, dtype=torch.int32, device=dev)
            sim.ep_i32 = torch.zeros((sim.P, 1, 8), dtype=torch.int32, device=dev)
            sim.ep_f64 = torch.zeros((sim.P, 1, 2), dtype=torch.float64, device=dev)
            sim._respawn = _lib.RespawnC(1, 0, sim.start_state.data_ptr(), sim.start_idx.data_ptr(), sim.due.data_ptr(), sim.served.data_ptr(),
                                         sim.ep_i32.data_ptr(), sim.ep_f64.data_ptr())
            sim._desc = None
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d%s'
                       % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, ', graph replay' if args.graph else ''),
           'steps': args.steps}
    for tag in tags:
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms = {t: [] for t in tags}
    parent = []
    last = {}
    child = None
    if args.parent_tree:
        tree = os.path.abspath(args.parent_tree)
        child = [sys.executable, os.path.join(tree, 'scripts', 'admit_timing.py'), '--reps', '1', '--only', 'admit_idle', '--steps', str(args.steps),
                 '--instances', str(args.instances), '--horizon', str(args.horizon)] + (['--graph'] if args.graph else [])
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
        if child:
            env = {k: v for k, v in os.environ.items() if k not in ('MPCX_LIB', 'PYTHONPATH')}
            out = subprocess.run(child, cwd=tree, env=env, check=True, capture_output=True, text=True)
            parent.append(json.loads(out.stdout.strip().splitlines()[-1])['admit_idle_median_ms_per_step'])
    for tag in tags:
        m, sim = np.array(ms[tag]), last[tag]
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_served'] = 0 if sim.served is None else sim.served_count()
        res[tag + '_waiting'] = sim.waiting_count()
    if parent:
        res['parent_admit_ms_per_step'] = [round(float(v), 4) for v in parent]
        res['parent_admit_median_ms_per_step'] = round(float(np.median(parent)), 4)
    if 'admit' in ms and 'respawn_idle' in ms:
        res['stage_overhead_ms_per_step'] = round(res['respawn_idle_median_ms_per_step'] - res['admit_median_ms_per_step'], 4)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
