"""Worker of the two-rank run-log rehearsal (spawned; it must live in an importable module)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def logged_agent_shard_worker(rank, world, port, B, steps, seed, out_path):
    """`world` ranks share cuda:0, rank r drives agents r * 8 / world .. of every instance with a run log attached; the pool rows travel
    over gloo through host memory (the staged path: mpcx_record_step_batch on the all-gathered pool).  Each rank saves its log."""
    import numpy as np
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    from mpc_for_av_at_intersection_amd.runtime import Context
    from mpc_for_av_at_intersection_amd.sharding import torch_exchange
    ctx = Context(0)
    sim = synthetic_batch(ctx, B=B, A=8, T=13, seed=seed, agent_shard=(rank, world), exchange=torch_exchange(world, 'cpu'))
    log = sim.attach_log(steps)
    sim.run(steps)
    sim.check()
    out = log.outcomes()
    np.savez(out_path % rank, rows=log.rows(), **out)
    dist.barrier()
    dist.destroy_process_group()
