"""GPU tests of the narrow mpcx_closed_loop_run* entry points, those up to admission, which nothing in the package calls:
Context.closed_loop_run always takes the widest one and passes NULL for what is off.  Each of them, called by itself through ctypes with
every struct it has a parameter for, directly and as a replayed graph, must leave the bits Context.closed_loop_run leaves with the same
structs -- in every buffer a step leaves (the array set and the bitwise test of tests/test_gpu_step_fusion.py; the work queue is left out
for the reason given there) and in the stages' own words.  The entry points from respawn upward are called by the tests of their stages."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_step_fusion as SF

pytestmark = pytest.mark.gpu
STEPS = 5
WAIT = np.array([-1, -1, 0, 2, -1, -1, 7, -1])      # two agents enter inside the run, one is still waiting at its end
# entry point -> the structs it takes beside the descriptor, in the order of its parameters
RUNGS = {
    'mpcx_closed_loop_run': (),
    'mpcx_closed_loop_run_logged': ('log',),
    'mpcx_closed_loop_run_opts': ('log', 'opts'),
    'mpcx_closed_loop_run_retire': ('log', 'opts', 'retire'),
    'mpcx_closed_loop_run_scene': ('log', 'opts', 'retire', 'scene'),
    'mpcx_closed_loop_run_admit': ('log', 'opts', 'retire', 'scene', 'admit'),
}
LOG_WORDS = ('rows_f64', 'rows_i32', 'steps', 'goal_step', 'contact_step', 'flags', 'min_clearance')
STAGE_WORDS = {'retire': ('done', 'steps_driven'), 'scene': ('absent',), 'admit': ('wait', 'entered_step', 'clock')}


@pytest.fixture(scope='module')
def ctx():
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def side():
    """(a replayed graph needs a stream of its own)"""
    from mpc_for_av_at_intersection_amd.runtime import Context
    c = Context(0, stream=torch.cuda.Stream(device=0))
    yield c
    c.close()


@pytest.fixture(scope='module')
def stock(ctx):
    from mpc_for_av_at_intersection_amd.batch import stock_routes
    return stock_routes(ctx)


def _batch(c, stock, stages):
    """one instance of 8 agents on the stock routes (one partial workgroup) with exactly the stages named switched on"""
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    routes, dl, cd = stock
    sim = synthetic_batch(c, B=1, A=8, T=20, seed=11, routes=routes, dl=dl, cd=cd, stop_mode='speed' if 'opts' in stages else 'cut')
    if 'log' in stages:
        sim.attach_log(STEPS)
    if 'retire' in stages:
        sim.retire_at_goal(leave_scene='scene' in stages)
    if 'admit' in stages:
        sim.enter_on_schedule(WAIT, gap=0.0)
    torch.cuda.synchronize()
    return sim


def _structs(sim):
    return sim._stage_structs()         # (every stage of _lib.STAGES: those beyond admission are off in every batch here)


def _call(sim, name, graph):
    """the entry point itself, with the structs of `sim` it has parameters for"""
    sim._claim_context()
    if sim._desc is None:
        sim._desc = sim._descriptor()
    cip, have, c = sim.ip.to_c(), _structs(sim), sim.ctx
    c._chk(getattr(c.lib, name)(c._ctx, C.byref(cip), C.byref(sim._desc), *(C.byref(have[k]) for k in RUNGS[name]), STEPS, int(graph)))
    c.synchronize()


def _words(sim, stages):
    out = {}
    if 'log' in stages:
        out.update({'log_' + k: getattr(sim.log, k) for k in LOG_WORDS})
    for st in stages:
        out.update({k: getattr(sim, k) for k in STAGE_WORDS.get(st, ())})
    return out


@pytest.mark.parametrize('name', list(RUNGS))
def test_entry_point_is_the_runtime_call(ctx, side, stock, name):
    stages = RUNGS[name]
    want = _batch(ctx, stock, stages)
    assert all((v is not None) == (k in stages) for k, v in _structs(want).items()), name
    want.run(STEPS)
    ctx.synchronize()
    assert (want.sol['iters'] > 0).any()
    if 'admit' in stages:       # the gate ran: its clock counts the steps, and a count-down of 7 has not ended in 5
        assert int(want.clock.item()) == STEPS and int(want.entered_step[6]) == -1 and int(want.done[6]) == 1
    for c, graph in ((ctx, False), (side, True)):
        got = _batch(c, stock, stages)
        _call(got, name, graph)
        SF._assert_same(got, want, '%s, graph %d' % (name, graph))
        a, b = _words(got, stages), _words(want, stages)
        for k in b:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, graph, k)
            assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), (name, graph, k)
