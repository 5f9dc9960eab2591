"""GPU box: what the run log costs and what it replaces.  For B = 4096, T = 20 and the first `steps` (100) steps of
scripted_traffic_batch(A = 1, K = 2) and (A = 8, K = 2), always from the START of the scenario and each variant on a fresh batch after a
throw-away copy has taken `warm` steps: ONE mpcx_closed_loop_run between two device barriers (a) without a log, (b) with a log of
capacity 0 (outcomes only), (c) with a log of capacity `steps`; the three are measured `rounds` (3) times in turn and the median is
reported.  Then (d) the same rows collected the old way: run(1) + snapshot() per step, wall time.  One JSON line per workload.
record_kernel's own time comes from a run of this script under `rocprofv3 --kernel-trace --stats -- python scripts/run_log_timing.py B
steps warm 1` (tracing only, a run of its own).

    python scripts/run_log_timing.py [B] [steps] [warm] [rounds]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch, stock_routes
from mpc_for_av_at_intersection_amd.runtime import Context

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
T = 20
ctx = Context(0)
routes, dl, cd = stock_routes(ctx)
kw = dict(T=T, seed=1000, routes=routes, dl=dl, cd=cd)


def timed(make, capacity):
    sim = make()
    log = None if capacity is None else sim.attach_log(capacity, max_bytes=None)
    ctx.synchronize()
    t0 = time.perf_counter()
    sim.run(STEPS)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    sim.check()
    out = None if log is None else log.outcomes()
    del sim, log
    torch.cuda.empty_cache()
    return 1e3 * wall / STEPS, out


for A in (1, 8):
    make = lambda: scripted_traffic_batch(ctx, B, A=A, K=2, **kw)
    sim = make()
    sim.attach_log(WARM, max_bytes=None)
    sim.run(WARM)
    sim.check()
    del sim
    ms = {'none': [], 'outcomes': [], 'rows': []}
    out = None
    for _ in range(ROUNDS):
        for name, cap in (('none', None), ('outcomes', 0), ('rows', STEPS)):
            t, o = timed(make, cap)
            ms[name].append(t)
            out = o if o is not None else out
    sim = make()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        sim.run(1)
        sim.snapshot()
    old_way = time.perf_counter() - t0
    del sim
    torch.cuda.empty_cache()
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({'workload': 'scripted A=%d K=2' % A, 'B': B, 'T': T, 'steps': STEPS, 'rounds': ROUNDS,
                      'ms_per_step_no_log': med['none'], 'ms_per_step_outcomes_only': med['outcomes'], 'ms_per_step_rows': med['rows'],
                      'all_ms_per_step': ms, 'log_bytes': B * A * (96 * STEPS + 24),
                      'run1_plus_snapshot_wall_s': old_way, 'logged_run_wall_s': 1e-3 * med['rows'] * STEPS,
                      'arrived': int((out['goal_step'] >= 0).sum()), 'contacts_after_separation': int((out['contact_step'] >= 0).sum()),
                      'worst_clearance_after_separation': float(out['min_clearance'].min())}), flush=True)
