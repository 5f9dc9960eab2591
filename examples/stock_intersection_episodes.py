#!/usr/bin/env python3
"""The reference's stock scenario (main/scenarios/mpc_intersection.py: one ego, two scripted cars that never yield) x B seeded variants
(batch.scripted_traffic_batch; instance 0 is the stock set itself), run as EPISODES: every ego is retired where the reference's loop ends
(`if mpc.is_goal(state): break`, scenarios/mpc_intersection.py:92-93; IntersectionBatch.retire_at_goal) and the batch runs until the last
one has arrived (run_until_done), with no host work between the steps of a chunk.  A retired ego is a parked car that is not solved, not
logged and not counted, so contacts and the worst clearance are those of the episode the reference would have run -- a scripted car that
passes a parked ego after its arrival is none -- and steps per episode is the reference's number of loop iterations.
examples/stock_intersection_batch.py runs the same family for a fixed number of steps without retirement.

    python examples/stock_intersection_episodes.py [--instances 1024] [--max-steps 400] [--chunk 16] [--horizon 20] [--graph]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=1024)
    ap.add_argument('--max-steps', type=int, default=400)
    ap.add_argument('--chunk', type=int, default=16, help='steps between two looks at the number of egos still driving')
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step as a hipGraph')
    args = ap.parse_args()

    import torch
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context

    ctx = Context(0, stream=torch.cuda.Stream(device=0)) if args.graph else Context(0)
    sim = scripted_traffic_batch(ctx, B=args.instances, T=args.horizon, seed=args.seed, A=1, K=2)
    log = sim.attach_log(0)                 # outcomes only: goal arrival, contact, worst clearance
    sim.retire_at_goal()                    # same goal_dis / stop_speed as the log: goal_step == steps_driven for every retired ego
    ctx.closed_loop_stats(reset=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    taken = sim.run_until_done(args.max_steps, chunk=args.chunk, graph=args.graph)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    sim.check()
    out = log.outcomes()
    done = sim.done.cpu().numpy() != 0
    driven = sim.steps_driven.cpu().numpy()
    assert np.array_equal(out['goal_step'][done], driven[done])
    touched = out['contact_step'] >= 0      # clearance < 0 after the ego had been clear of everybody, DURING its episode
    seen = np.isfinite(out['min_clearance'])
    stats = ctx.closed_loop_stats()
    ep = driven[done]
    print('%d episodes on the device, %d steps taken in %.3f s (%.0f agent-steps solved, %.1f %% of instances x steps): %d of %d egos arrived; '
          'steps per episode min / median / max %s; %d egos touched a vehicle during their episode, worst clearance %.2f m; %d QP failures; '
          'stock instance: %d steps (the reference: 79 at T = 20)'
          % (args.instances, taken, wall, stats['agent_steps'], 100.0 * stats['agent_steps'] / max(args.instances * taken, 1), int(done.sum()),
             len(done), '%d / %d / %d' % (ep.min(), np.median(ep), ep.max()) if len(ep) else '- / - / -', int(touched.sum()),
             float(out['min_clearance'][seen].min()) if seen.any() else float('inf'), stats['failures'], int(driven[0])))


if __name__ == '__main__':
    main()
