"""GPU box: what a closed-loop step costs in the two stop modes.  The seeded family scripted_traffic_batch(B = 4096, A = 1, K = 2) -- the
reference's scenario with its two scripted cars -- and scripted_traffic_batch(A = 8, K = 2), each with stop_mode 'cut' and 'speed', all four
with the controller constants of lib/mpc_with_speed.py (T = 13, speed weight 20), so that the mode is the only difference within a pair.
Per workload, always from the START of the scenario: a throw-away copy takes `warm` steps (allocations, first launches); a fresh copy
takes its first `steps` steps in ONE call between two device barriers (timesteps/s = instance-steps per second, ms per step, mean
interior-point iterations per QP, failed solves); arrivals, contacts and the worst clearance come from a run log with capacity 0 on a
third copy.  One JSON line per workload.

    python scripts/speedref_timing.py [B] [steps] [warm]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, stock_routes
from mpc_for_av_at_intersection_amd.lib import mpc_with_speed
from mpc_for_av_at_intersection_amd.runtime import Context

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = Context(0)
routes, dl, cd = stock_routes(ctx)
params = mpc_with_speed.params(cd, 0.2)
kw = dict(seed=1000, routes=routes, dl=dl, cd=cd, mpc=params)
for A in (1, 8):
    for mode in ('cut', 'speed'):
        make = lambda: scripted_traffic_batch(ctx, B, A=A, K=2, stop_mode=mode, **kw)
        sim = make()
        sim.run(WARM)
        sim.check()
        del sim
        sim = make()
        ctx.synchronize()
        ctx.closed_loop_stats(reset=True)
        t0 = time.perf_counter()
        sim.run(STEPS)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        st = ctx.closed_loop_stats(reset=True)
        sim.check()
        v = sim.state[:, 2]
        speed, standing = float(v.mean().item()), float((v.abs() < 0.1).double().mean().item())
        del sim
        sim = make()
        log = sim.attach_log(0)
        sim.run(STEPS)
        out = log.outcomes()
        seen = np.isfinite(out['min_clearance'])
        print(json.dumps({'workload': 'scripted A=%d K=2' % A, 'stop_mode': mode, 'B': B, 'A': A, 'T': params.T, 'steps': STEPS,
                          'timesteps_per_s': B * STEPS / wall, 'ms_per_step': 1e3 * wall / STEPS,
                          'mean_ipm_iters': st['iterations'] / max(st['agent_steps'], 1), 'qp_failures': st['failures'],
                          'arrived': int((out['goal_step'] >= 0).sum()), 'touched': int((out['contact_step'] >= 0).sum()),
                          'worst_clearance': float(out['min_clearance'][seen].min()) if seen.any() else None,
                          'mean_ego_speed_at_end': speed, 'standing_share_at_end': standing}), flush=True)
        del sim, log
        torch.cuda.empty_cache()
