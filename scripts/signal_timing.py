#!/usr/bin/env python3
"""What traffic signals cost per step: the routed respawn batch of scripts/precedence_timing.py (instances x 8 agents on the eight stock
routes, all from the first point of their route, the seeded demand of batch.demand_schedule(), every slot kept on its own route) in three
variants:

    off       no signals (mpcx_closed_loop_run_routes)
    green     signalise() with every group green for the whole cycle: signal_kernel runs, nobody is ever held -- the run is the `off` run
              bit for bit, so the difference is the stage's own cost (one more dependent launch per step)
    plan      signalise(two_phase_plan(cycle, green, amber)): traffic that flows differently

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run; reported: median and range of
the time per step.  Then the `plan` variant once more, step by step without a graph and with the QP launches bracketed by events
(Context.profile_qp): the QP launch time and the largest iteration count of the steps in which a light changes -- where the agents were
filed in the QP work queue under a key from the cut BEFORE the signal stage -- against the steps in which none does.

    python scripts/signal_timing.py [--reps 3] [--steps 150] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0] [--graph]
                                    [--cycle 100] [--green 30] [--amber 8] [--probe-steps 300]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

TAGS = ('off', 'green', 'plan')


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
    ap.add_argument('--cycle', type=int, default=100)
    ap.add_argument('--green', type=int, default=30)
    ap.add_argument('--amber', type=int, default=8)
    ap.add_argument('--probe-steps', type=int, default=300, help='steps of the step-by-step run that times the QP launches (0: skip it)')
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, two_phase_plan
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    plan = two_phase_plan(args.cycle, args.green, args.amber)
    all_green = dict(cycle=args.cycle, amber=0, green=np.array([[0, args.cycle]] * 4))

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
        if tag != 'off':
            sim.signalise(all_green if tag == 'green' else plan)
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d, plan %d / %d / %d%s'
                       % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, args.cycle, args.green, args.amber,
                          ', graph replay' if args.graph else ''),
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
    res['green_minus_off_ms_per_step'] = round(res['green_median_ms_per_step'] - res['off_median_ms_per_step'], 4)
    res['plan_minus_off_ms_per_step'] = round(res['plan_median_ms_per_step'] - res['off_median_ms_per_step'], 4)
    a, b = last['off'], last['green']
    res['green_is_the_off_run'] = bool(a.episodes().tobytes() == b.episodes().tobytes() and a.state.cpu().numpy().tobytes() == b.state.cpu().numpy().tobytes())
    res['plan_held_at_end'] = int((last['plan'].held != 0).sum().item())
    if args.probe_steps > 0 and not args.graph:
        # the light of either phase at tick t against tick t - 1: the steps in which a light changes

        def light(g, t):
            u = (t - int(plan['green'][g][0])) % args.cycle
            return 0 if u < int(plan['green'][g][1]) else 1 if u < int(plan['green'][g][1]) + args.amber else 2
        sim = fresh('plan')
        ctx.closed_loop_stats(reset=True)
        ctx.profile_qp(True)
        rows = {True: [], False: []}
        try:
            for s in range(args.probe_steps):
                sim.run(1)
                ctx.synchronize()
                qp_ms, launches = ctx.profile_qp_read()
                st = ctx.closed_loop_stats(reset=True)
                t = s % args.cycle
                changed = s > 0 and any(light(g, t) != light(g, (t - 1) % args.cycle) for g in range(4))
                rows[changed].append((qp_ms, st['max_iterations'], st['iterations'] / max(1, st['agent_steps'])))
        finally:
            ctx.profile_qp(False)
        for key, name in ((True, 'change'), (False, 'steady')):
            r = np.array(rows[key]) if rows[key] else np.zeros((0, 3))
            res['qp_%s_steps' % name] = len(r)
            if len(r):
                res['qp_%s_ms_median' % name], res['qp_%s_ms_min' % name], res['qp_%s_ms_max' % name] = (round(float(v), 4) for v in (np.median(r[:, 0]), r[:, 0].min(), r[:, 0].max()))
                res['qp_%s_max_iterations' % name] = int(r[:, 1].max())
                res['qp_%s_mean_iterations' % name] = round(float(r[:, 2].mean()), 3)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
