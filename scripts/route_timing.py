#!/usr/bin/env python3
"""What routing costs per step, and what the device summary saves: the open-intersection batch (examples/open_intersection_flow.py:
instances x 8 agents on the eight stock routes, all from the first point of their route) with the seeded demand of batch.demand_schedule()
in both variants:

    respawn   respawn_on_schedule(due, gap): a slot keeps its route (respawn_kernel ends the step)
    routed    the same schedule with route= given and every slot kept on its own route (respawn_route_kernel ends the step instead: the same
              number of launches, the same vehicles on the same routes -- the two runs must serve the same episodes)

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step.  Then mpcx_episode_summary on an episode table of instances x 8 slots x --table-vehicles vehicles (random finished
records on the eight routes): HIP events around --summary-reps launches, beside the wall time of copying the table (served, ep_i32, ep_f64)
to the host.

    python scripts/route_timing.py [--reps 3] [--steps 150] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0] [--graph]
                                   [--table-vehicles 16] [--summary-reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))

TAGS = ('respawn', 'routed')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    ap.add_argument('--vehicles', type=int, default=3)
    ap.add_argument('--gap', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--table-vehicles', type=int, default=16)
    ap.add_argument('--summary-reps', type=int, default=20)
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        own = np.repeat(route[:, :, None], args.vehicles, axis=2) if tag == 'routed' else None
        sim.respawn_on_schedule(due, gap=args.gap, route=own)
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d%s'
                       % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, ', graph replay' if args.graph else ''),
           'steps': args.steps}
    for tag in TAGS:
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms, last = {t: [] for t in TAGS}, {}
    for _ in range(args.reps):
        for tag in TAGS:
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
    for tag in TAGS:
        m, sim = np.array(ms[tag]), last[tag]
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_served'] = sim.served_count()
    res['routed_minus_respawn_ms_per_step'] = round(res['routed_median_ms_per_step'] - res['respawn_median_ms_per_step'], 4)
    a, b = last['respawn'], last['routed']
    res['same_episodes'] = bool(a.episodes().tobytes() == b.episodes().tobytes())
    tab = b.movement_summary()
    res['routed_episodes_per_route'] = [int(v) for v in tab['count'].sum(axis=0)]

    # the summary on a full-size table beside the copy it replaces
    rng = np.random.default_rng(args.seed)
    P, G = args.instances * 8, args.table_vehicles
    w = rng.integers(0, 400, (P, G, 8)).astype(np.int32)
    w[:, :, 7] = rng.integers(0, 8, (P, G))
    served, ep_i32 = ctx.i32(rng.integers(0, G + 1, P)), ctx.i32(w)
    ep_f64 = ctx.f64(rng.uniform(-1.0, 5.0, (P, G, 2)))
    ctx.episode_summary(8, 8, served, ep_i32, ep_f64)       # warm-up
    ctx.synchronize()
    stream = torch.cuda.current_stream(ctx.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.summary_reps):       # (every call also fills its two small output tensors: two more tiny launches)
        out = ctx.episode_summary(8, 8, served, ep_i32, ep_f64)
    e1.record(stream)
    e1.synchronize()
    ctx.synchronize()
    res['summary_ms_per_call'] = round(e0.elapsed_time(e1) / args.summary_reps, 4)
    copies = []
    for _ in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        host = [t.cpu() for t in (served, ep_i32, ep_f64)]
        copies.append((time.perf_counter() - t0) * 1e3)
    res['table_copy_ms'] = [round(v, 3) for v in copies]
    res['table_bytes'] = int(sum(t.numel() * t.element_size() for t in host))
    res['summary_bytes'] = int(sum(t.numel() * t.element_size() for t in out))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
