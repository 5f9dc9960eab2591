"""GPU box: what the closed loop costs and does with the reference's own scripted cars in it.  For B = 4096, T = 20:
(a) scripted_traffic_batch(A = 1, K = 2) -- the stock scenario as a seeded family, (b) scripted_traffic_batch(A = 8, K = 2), next to
(c) synthetic_batch(A = 8) -- eight egos that all yield to each other, no scripted car.  Per workload, always from the START of the
scenario (the stock scenario is over after ~80 steps: later steps only see egos standing at the end of their paths): a throw-away copy
takes `warm` steps (allocations, first launches); a fresh copy takes its first 100 steps in ONE mpcx_closed_loop_run between two device
barriers (timesteps/s = instance-steps per second, ms per step, mean interior-point iterations per QP); a third copy takes the same 100
steps ten at a time for what cannot be had inside a timed stretch: QP launch time (HIP events around every QP launch), share of the QPs
the trial pass solves, mean ego speed and share of standing egos (|v| < 0.1 m/s), each sampled after every tenth step.  One JSON line
per workload.

    python scripts/scripted_traffic_timing.py [B] [steps] [warm]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, stock_routes, synthetic_batch
from mpc_for_av_at_intersection_amd.runtime import Context

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 20
T = 20
ctx = Context(0)
routes, dl, cd = stock_routes(ctx)
kw = dict(T=T, seed=1000, routes=routes, dl=dl, cd=cd)
workloads = [('scripted A=1 K=2', lambda: scripted_traffic_batch(ctx, B, A=1, K=2, **kw)),
             ('scripted A=8 K=2', lambda: scripted_traffic_batch(ctx, B, A=8, K=2, **kw)),
             ('synthetic A=8', lambda: synthetic_batch(ctx, B, A=8, **kw))]
for name, make in workloads:
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
    del sim
    sim = make()
    ctx.profile_qp(True); ctx.profile_qp_read()
    speed, standing, trial = [], [], []
    for _ in range(STEPS // 10):
        sim.run(10)
        v = sim.state[:, 2]
        speed.append(float(v.mean().item())); standing.append(float((v.abs() < 0.1).double().mean().item()))
        trial.append(float(((sim.sol['iters'] == 0) & (sim.sol['status'] == 0)).double().mean().item()))
    qp_ms, qp_n = ctx.profile_qp_read()
    ctx.profile_qp(False)
    mean = lambda a: sum(a) / len(a)
    print(json.dumps({'workload': name, 'B': B, 'A': sim.A, 'K': 0 if sim.traffic is None else int(sim.traffic.k_of_instance.max()), 'T': T,
                      'steps': STEPS, 'timesteps_per_s': B * STEPS / wall, 'ms_per_step': 1e3 * wall / STEPS,
                      'qp_launch_ms': qp_ms / max(qp_n, 1), 'mean_ipm_iters': st['iterations'] / max(st['agent_steps'], 1),
                      'qp_failures': st['failures'], 'qp_solved_by_trial_pass': mean(trial),
                      'mean_ego_speed': mean(speed), 'standing_share': mean(standing)}), flush=True)
    del sim
    torch.cuda.empty_cache()
