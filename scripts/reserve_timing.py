#!/usr/bin/env python3
"""What the reservation stage costs beside the actuated signal stage: the respawn batch of scripts/actuated_timing.py (instances x 8 agents
on the eight stock routes, the seeded demand of batch.demand_schedule()) in three variants:

    off       no signals
    actuated  actuate(two_phase_controller(...)): actuated_signal_kernel, a lane group of 8 per junction
    reserved  reserve(dict(detect, patience)): reserve_kernel in its place, the same lane group -- the same number of launches per step

The variants alternate within every repetition, after a warm-up run of each; HIP events around the whole run(steps); reported: median and
range of the time per step, and the stage's own cost against the run without signals.  Then the two stage calls alone
(Context.actuated_step, Context.reserve_step) on the words of the last runs, `--stage-reps` launches back to back between two events.
The kernel's own time comes from a run of its own under the profiler, which this script does not start:

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/reserve_timing.py --only reserved --reps 1 --stage-reps 0

    python scripts/reserve_timing.py [--reps 3] [--steps 100] [--instances 4096] [--headway 25] [--vehicles 3] [--gap 2.0] [--graph]
                                     [--min-green 10] [--max-green 60] [--gap-out 5] [--amber 8] [--all-red 12] [--detect 100]
                                     [--patience 0] [--stage-reps 200] [--only TAG]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

TAGS = ('off', 'actuated', 'reserved')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--instances', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=13)
    ap.add_argument('--headway', type=float, default=25.0)
    ap.add_argument('--vehicles', type=int, default=3)
    ap.add_argument('--gap', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--min-green', type=int, default=10)
    ap.add_argument('--max-green', type=int, default=60)
    ap.add_argument('--gap-out', type=int, default=5)
    ap.add_argument('--amber', type=int, default=8)
    ap.add_argument('--all-red', type=int, default=12)
    ap.add_argument('--detect', type=int, default=100)
    ap.add_argument('--patience', type=int, default=0, help='steps a denied request waits before it blocks later ones; negative: unbounded')
    ap.add_argument('--stage-reps', type=int, default=200, help='launches of either stage kernel alone between two events (0: skip)')
    ap.add_argument('--only', choices=TAGS, default=None, help='run this variant alone (for a profiler run of its own)')
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    import torch
    from open_intersection_flow import family
    from mpc_for_av_at_intersection_amd.batch import demand_schedule, stock_routes, two_phase_controller
    from mpc_for_av_at_intersection_amd.runtime import Context
    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    routes, dl, cd = stock_routes(ctx)
    ctrl = two_phase_controller(args.min_green, args.max_green, args.gap_out, args.amber, args.all_red, args.detect)
    mgr = dict(detect=args.detect, patience=None if args.patience < 0 else args.patience)
    tags = TAGS if args.only is None else (args.only,)

    def fresh(tag):
        sim, route = family(ctx, routes, dl, cd, args.instances, args.horizon)
        sim.retire_at_goal(leave_scene=True)
        due = demand_schedule(route, routes, np.zeros_like(route), args.headway, args.vehicles, args.seed)
        sim.respawn_on_schedule(due, gap=args.gap, route=np.repeat(route[:, :, None], args.vehicles, axis=2))
        if tag == 'actuated':
            sim.actuate(ctrl)
        elif tag == 'reserved':
            sim.reserve(mgr)
        return sim
    res = {'workload': 'open intersection %d x 8, T = %d, headway %.1f, %d vehicles per slot, gap %.1f, seed %d, controller %d / %d / %d / %d / %d, '
                       'detector %d, patience %s%s' % (args.instances, args.horizon, args.headway, args.vehicles, args.gap, args.seed, args.min_green,
                                                       args.max_green, args.gap_out, args.amber, args.all_red, args.detect, mgr['patience'],
                                                       ', graph replay' if args.graph else ''),
           'steps': args.steps}
    for tag in tags:
        fresh(tag).run(args.steps, args.graph)      # warm-up
    ctx.synchronize()
    ms, last = {t: [] for t in tags}, {}
    stream = torch.cuda.current_stream(ctx.device)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ctx.synchronize()
        return e0.elapsed_time(e1) / n
    for _ in range(args.reps):
        for tag in tags:
            sim = fresh(tag)
            ctx.synchronize()
            ms[tag].append(timed(lambda: sim.run(args.steps, args.graph), args.steps))
            last[tag] = sim
    for tag in tags:
        m, sim = np.array(ms[tag]), last[tag]
        res[tag + '_ms_per_step'] = [round(float(v), 4) for v in m]
        res[tag + '_median_ms_per_step'], res[tag + '_min'], res[tag + '_max'] = round(float(np.median(m)), 4), round(float(m.min()), 4), round(float(m.max()), 4)
        res[tag + '_served'] = sim.served_count()
        if tag != 'off':
            res[tag + '_held_at_end'] = int((sim.held != 0).sum().item())
    if 'off' in tags:
        for tag in tags[1:]:        # the stage's own cost: per repetition against the run without signals of the same repetition
            d = 1000.0 * (np.array(ms[tag]) - np.array(ms['off']))
            res[tag + '_stage_us_per_step'] = [round(float(v), 2) for v in d]
            res[tag + '_stage_median_us_per_step'] = round(float(np.median(d)), 2)
    if 'reserved' in tags:
        res['reserved_queued_at_end'], res['reserved_granted_at_end'] = int(last['reserved'].queued.sum().item()), int(last['reserved'].granted.sum().item())
        res['reserved_max_queued_in_a_junction'] = int(last['reserved'].queued.max().item())
    if args.stage_reps > 0 and args.only is None:   # either kernel alone on the words its run left (the junction words move on: harmless here)
        n = args.stage_reps
        a, b = last['actuated'], last['reserved']
        cut_a, cut_b = a.inter['cut_len'].clone(), b.inter['cut_len'].clone()

        def actuated_stage():
            for _ in range(n):
                ctx.actuated_step(a.dl, a.state, a.path_off, a.path_len, a.traj_idx, cut_a, a._signals, a._actuation, done=a.done)

        def reserve_stage():
            for _ in range(n):
                ctx.reserve_step(b.dl, b.state, b.path_off, b.path_len, b.traj_idx, cut_b, b._signals, b._reservation, done=b.done)
        actuated_stage(); reserve_stage(); ctx.synchronize()      # warm-up
        us = {'actuated_signal_kernel': [], 'reserve_kernel': []}
        for _ in range(args.reps):
            us['actuated_signal_kernel'].append(1000.0 * timed(actuated_stage, n))
            us['reserve_kernel'].append(1000.0 * timed(reserve_stage, n))
        for k, v in us.items():
            res[k + '_us_per_call'] = [round(float(x), 3) for x in v]
            res[k + '_median_us_per_call'] = round(float(np.median(v)), 3)
        res['stage_note'] = 'back-to-back stage calls from the host, each with its struct check (the three small tables read back): an upper bound of the launch'
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
