#!/usr/bin/env python3
"""What the advice stage costs per step: the open intersection of scripts/signal_timing.py in speed mode (instances x 8 agents on the eight
stock routes, all from the first point of their route, the seeded demand of batch.demand_schedule() through the admission gate, every slot
kept on its own route) under signalise(two_phase_plan(cycle, green, amber)) with seeded clocks, in three variants:

    signals   signalise() alone (mpcx_closed_loop_run_signals' launches)
    idle      + advise_speed(reach=1e-6): advise_kernel runs between the window stage and the QP of every step and nobody is ever within
              reach -- the run is the `signals` run bit for bit, so the difference is the stage's own cost (one more dependent launch)
    advice    + advise_speed(): traffic that flows differently (capped speed references are other QPs)

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step, the differences, and how many agent-steps of the last step were advised.

    python scripts/advise_timing.py [--reps 5] [--steps 150] [--instances 4096] [--horizon 13] [--headway 25] [--vehicles 3] [--gap 2.0]
                                    [--cycle 100] [--green 30] [--amber 8] [--graph]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAGS = ('signals', 'idle', 'advice')


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
    ap.add_argument('--cycle', type=int, default=100)
    ap.add_argument('--green', type=int, default=30)
    ap.add_argument('--amber', type=int, default=8)
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from mpc_for_av_at_intersection_amd.batch import IntersectionBatch, demand_schedule, stock_routes, two_phase_plan
    from mpc_for_av_at_intersection_amd.lib import mpc_with_speed
    from mpc_for_av_at_intersection_amd.runtime import Context, InteractionParams
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    plan = two_phase_plan(args.cycle, args.green, args.amber)
    offset = np.random.default_rng(args.seed).integers(0, args.cycle, args.instances)
    route = np.tile(np.arange(8), (args.instances, 1))
    ip = InteractionParams(cutoff_margin=4 * int(np.ceil(cd.radius / dl)), L=cd.distance_back_to_front_wheel, radius=cd.radius,
                           circle_centers=np.asarray(cd.circle_centers).ravel())
    params = dataclasses.replace(mpc_with_speed.params(cd, 0.2), T=args.horizon, L=cd.distance_back_to_front_wheel)

    def fresh(tag):
        sim = IntersectionBatch(ctx, params, ip, routes, dl, route, np.zeros_like(route), stop_mode='speed')
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
        sim.signalise(plan, offset=offset)
        if tag == 'idle':
            sim.advise_speed(reach=1e-6)
        elif tag == 'advice':
            sim.advise_speed()
        return sim
    res = {'workload': 'open intersection in speed mode, %d x 8 signalised agents, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d, '
                       'plan %d / %d / %d%s' % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, args.cycle,
                                                args.green, args.amber, ', graph replay' if args.graph else ''),
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
        m = np.array(ms[tag])
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_held_at_end'] = int((last[tag].held != 0).sum().item())
        res[tag + '_served'] = last[tag].served_count()
    res['idle_minus_signals_ms_per_step'] = round(res['idle_median_ms_per_step'] - res['signals_median_ms_per_step'], 4)
    res['idle_is_the_signals_run'] = bool(last['idle'].state.cpu().numpy().tobytes() == last['signals'].state.cpu().numpy().tobytes() and
                                          not last['idle'].advised.any().item())
    res['advice_minus_signals_ms_per_step'] = round(res['advice_median_ms_per_step'] - res['signals_median_ms_per_step'], 4)
    res['advised_at_end'] = int((last['advice'].advised > 0).sum().item())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
