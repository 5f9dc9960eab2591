"""The run log without a GPU: the host build of csrc/mpcx_record_core.h (the rule record_kernel runs one lane per agent at the end of a
closed-loop step) fed with the reference's recorded stock runs -- goal arrival = the reference's loop length, xref_deviation against
the formula of mpc.py:301-308, clearance against numpy with the two scripted cars of the stock scenario --, hand-made contact cases,
the sanitizers, the ctypes mirrors and the overflow rule.  The device side is tests/test_gpu_runlog.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests.test_traffic_cpu import golden_vehicles

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'record_ref', 'record_ref.cpp')
INC = ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc')]
GOAL_DIS, STOP_SPEED = 1.5, 0.1389        # lib/mpc.py

# (file, horizon, the reference's number of loop iterations or -1 = it never arrived, linearisation passes per step)
STOCK_RUNS = [('closedloop.npz', 10, 82, 1), ('closedloop.npz', 13, 82, 1), ('closedloop.npz', 20, 79, 1),
              ('closedloop_horizons.npz', 16, 81, 1), ('closedloop_horizons.npz', 24, 80, 1), ('closedloop_horizons.npz', 32, 79, 1),
              ('closedloop_iter2.npz', 13, -1, 2)]


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('record_ref') / 'librecord_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    from mpc_for_av_at_intersection_amd import _lib
    lib.record_ref_step.restype = None
    lib.record_ref_step.argtypes = ([C.POINTER(_lib.InteractionParamsC), C.c_int, C.c_int] + [C.c_void_p] * 12 + [C.c_int] + [C.c_void_p] * 4 +
                                    [C.POINTER(_lib.RunLogC)])
    lib.record_ref_selfcase.restype = None
    lib.record_ref_selfcase.argtypes = [C.c_void_p]
    return lib


def car():
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    return BicycleModelDimensions()


class HostLog:
    """mpcx_run_log over numpy arrays + the call of the host build for one step of P agents"""

    def __init__(self, lib, P, capacity, T, radius, centers, goal_dis=GOAL_DIS, stop_speed=STOP_SPEED):
        from mpc_for_av_at_intersection_amd import _lib
        self.lib, self.P, self.cap, self.T = lib, P, capacity, T
        self.rows_f64 = np.full((max(capacity, 1), P, 8), -7.0)
        self.rows_i32 = np.full((max(capacity, 1), P, 8), -7, np.int32)
        self.steps, self.flags = np.zeros(P, np.int32), np.zeros(P, np.int32)
        self.goal_step, self.contact_step = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
        self.min_clearance = np.full(P, np.inf)
        self.c = _lib.RunLogC()
        self.c.capacity, self.c.goal_dis, self.c.stop_speed = capacity, goal_dis, stop_speed
        for n in ('rows_f64', 'rows_i32', 'steps', 'goal_step', 'contact_step', 'flags', 'min_clearance'):
            setattr(self.c, n, getattr(self, n).ctypes.data)
        self.ip = _lib.InteractionParamsC()
        self.ip.radius = radius
        self.ip.circle_centers[:] = list(np.asarray(centers, dtype=np.float64).ravel())

    def step(self, state, applied, x_sol, path, path_off, path_len, target, cut, pool, obs_off, obs_cnt, obs_skip, tidx=None, hit=None,
             status=None, iters=None):
        P = self.P
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
        i = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(0 if a is None else a, dtype=np.int32), (P,)))
        keep = [f(state, (P, 4)), f(applied, (P, 2)), f(x_sol, (P, 4, self.T + 1)), f(path, (-1, 3)), i(path_off), i(path_len), i(target), i(cut),
                i(tidx), i(hit), i(status), i(iters)]
        pool = f(pool, (-1, 6))
        tail = [pool, i(obs_off), i(obs_cnt), i(obs_skip)]
        self.lib.record_ref_step(C.byref(self.ip), P, self.T, *[a.ctypes.data for a in keep], len(pool), *[a.ctypes.data for a in tail], C.byref(self.c))


def stock_run(name, T, passes):
    """the arrays the rule reads, per step of a recorded stock run: post-step state i = recorded state[i + 1], the last one from
    lib.simulation.Simulation.step on the last recorded state and control"""
    from mpc_for_av_at_intersection_amd.lib.simulation import Simulation, State
    g = H.gold(name)
    pre = 'T%d/' % T
    state, ctrl = g[pre + 'state'], g[pre + 'ctrl']                 # (x, y, v, yaw) before each step; (steer, accel) applied in it
    x, y, v, yaw = state[-1]
    last = Simulation(car(), 0.2, State(x=x, y=y, yaw=yaw, v=v)).step(ctrl[-1][1], ctrl[-1][0])
    post = np.concatenate([state[1:], [[last.x, last.y, last.v, last.yaw]]])
    sel = slice(passes - 1, None, passes)                           # the solution and status of a step's LAST linearisation pass
    return dict(n=len(state), pre=state, post=post, ctrl=ctrl, ox=g[pre + 'ox'][sel], status=g[pre + 'status'][sel], target=g[pre + 'target'],
                cut=g[pre + 'cut'], full=g[pre + 'full'], steps=int(g[pre + 'steps']), tidx=g[pre + 'tidx'])


def feed(ref, run, T, capacity, cars=None):
    """one agent: the run through the rule.  cars: (n, K, 6) rows of scripted cars sharing the ego's pool window, or None = the ego alone"""
    cd = car()
    log = HostLog(ref, 1, capacity, T, cd.radius, cd.circle_centers)
    K = 0 if cars is None else cars.shape[1]
    for i in range(run['n']):
        prev = run['ctrl'][i - 1] if i else np.zeros(2)
        ego = np.concatenate([run['pre'][i], [prev[1], prev[0]]])
        pool = ego[None] if cars is None else np.concatenate([ego[None], cars[i]])
        log.step(run['post'][i], run['ctrl'][i], run['ox'][i], run['full'], 0, len(run['full']), run['target'][i], run['cut'][i], pool, 0, 1 + K, 0,
                 tidx=run['tidx'][i], status=run['status'][i])
    return log


@pytest.mark.parametrize('name,T,want,passes', STOCK_RUNS)
def test_goal_arrival_is_the_references_loop_length(ref, name, T, want, passes):
    """goal_step of the recorded stock runs = the golden's `steps` (82, 82, 79, 81, 80, 79 iterations of the reference's loop); the run with
    two linearisation passes was stopped after 59 steps, 16.7 m from the goal: -1.  The comparisons are far from their thresholds on every
    step (the margins are asserted), so the device, whose states differ from these by up to 1e-6, must find the same numbers."""
    run = stock_run(name, T, passes)
    log = feed(ref, run, T, capacity=0)
    assert int(log.goal_step[0]) == want, (T, log.goal_step)
    assert int(log.steps[0]) == run['n']
    if want >= 0:
        assert want == run['steps'] == run['n']
    goal = run['full'][-1]
    d = np.hypot(run['post'][:, 0] - goal[0], run['post'][:, 1] - goal[1])
    assert np.abs(d - GOAL_DIS).min() > 1e-3 and np.abs(np.abs(run['post'][:, 2]) - STOP_SPEED).min() > 1e-4
    # capacity 0: nothing but the outcome words was written
    assert (log.rows_f64 == -7.0).all() and (log.rows_i32 == -7).all()
    assert np.isinf(log.min_clearance[0]) and log.contact_step[0] == -1 and log.flags[0] == 1


@pytest.mark.parametrize('T', [10, 13, 20])
def test_xref_deviation_is_the_references_formula(ref, T):
    """mpc.py:301-308 with numpy on the same goldens (full[target], ox[:, :2, 0]): within 1e-12; the maxima are decimetres, not zeros"""
    run = stock_run('closedloop.npz', T, 1)
    log = feed(ref, run, T, capacity=run['n'])
    rows = log.rows_f64[:run['n'], 0]
    pt = run['full'][run['target']]
    ang = pt[:, 2] + np.pi / 2
    want = np.hypot(np.cos(ang) * (pt[:, 0] - run['ox'][:, 0, 0]), np.sin(ang) * (pt[:, 1] - run['ox'][:, 1, 0]))
    assert (run['status'] == 0).all()
    assert np.abs(rows[:, 6] - want).max() <= 1e-12
    assert 0.15 < want.max() < 0.7
    # the class's own expression, on a few steps
    from mpc_for_av_at_intersection_amd.lib.mpc import MPC
    for i in (0, 7, run['n'] - 1):
        m = MPC.__new__(MPC)
        m.cx, m.cy, m.cyaw, m.target_ind = run['full'][:, 0], run['full'][:, 1], run['full'][:, 2], int(run['target'][i])
        m.ox, m.oy = run['ox'][i, 0], run['ox'][i, 1]
        assert abs(m.get_current_xref_deviation() - rows[i, 6]) <= 1e-12
    # the other columns are copies
    assert np.array_equal(rows[:, :4], run['post']) and np.array_equal(rows[:, 4], run['ctrl'][:, 1]) and np.array_equal(rows[:, 5], run['ctrl'][:, 0])
    ints = log.rows_i32[:run['n'], 0]
    assert np.array_equal(ints[:, 0], run['tidx']) and np.array_equal(ints[:, 1], run['target']) and np.array_equal(ints[:, 2], run['cut'])
    assert not ints[:, 6:].any()
    # a failed solve has no solution to measure from: NaN, History.store's "no value"
    cd = car()
    one = HostLog(ref, 1, 1, T, cd.radius, cd.circle_centers)
    one.step(run['post'][0], run['ctrl'][0], run['ox'][0], run['full'], 0, len(run['full']), run['target'][0], run['cut'][0],
             np.zeros((1, 6)), 0, 1, 0, status=1)
    assert np.isnan(one.rows_f64[0, 0, 6]) and one.rows_i32[0, 0, 4] == 1


def numpy_clearance(ego_pose, others, cd):
    """min over the other vehicles and the disc pairs of the centre distance, - 2 radius (poses: rows x, y, yaw)"""
    from mpc_for_av_at_intersection_amd.lib.trajectories import car_trajectory_to_collision_point_trajectories as discs
    if len(others) == 0:
        return np.inf
    e = [d[0, :2] for d in discs(np.atleast_2d(ego_pose), cd)]
    o = [d[:, :2] for d in discs(np.atleast_2d(others), cd)]
    return min(float(np.hypot(*(a - b).T).min()) for a in e for b in o) - 2 * cd.radius


def outcome_from_clearances(c):
    """(contact_step, min_clearance) 'after separation' from a sequence of clearances"""
    clear = np.nonzero(c >= 0)[0]
    if len(clear) == 0:
        return -1, np.inf
    tail = c[clear[0]:]
    hit = np.nonzero(tail < 0)[0]
    return (int(clear[0] + hit[0]) if len(hit) else -1), float(tail.min())


def test_clearance_on_the_stock_run_with_its_two_cars(ref):
    """T = 13 with the cars of scenarios/mpc_intersection.py:42-45 from lib.moving_obstacles: the second car spawns ON the ego's start pose
    (clearance -2 radius at step 0) and the two separate for good, so contact_step = -1 and min_clearance = the numpy minimum over the
    steps from the first clear one on"""
    cd = car()
    run = stock_run('closedloop.npz', 13, 1)
    objs = [o for n, o, _ in golden_vehicles() if n.startswith('stock')]
    cars = np.stack([o.tape(run['n']) for o in objs], axis=1)
    log = feed(ref, run, 13, capacity=run['n'], cars=cars)
    got = log.rows_f64[:run['n'], 0, 7]
    want = np.array([numpy_clearance(run['pre'][i][[0, 1, 3]], cars[i][:, [0, 1, 3]], cd) for i in range(run['n'])])
    assert np.abs(got - want).max() <= 1e-12
    assert abs(got[0] + 2 * cd.radius) <= 1e-12
    first_clear = int(np.nonzero(got >= 0)[0][0])
    assert first_clear == 25 and (got[:first_clear] < 0).all() and got[first_clear:].min() > 1.0      # below 0 for the car's 4-s start delay + 5 steps
    contact, minc = outcome_from_clearances(got)
    assert contact == -1 == int(log.contact_step[0])
    assert abs(float(log.min_clearance[0]) - want[first_clear:].min()) <= 1e-12 and float(log.min_clearance[0]) == minc
    assert int(log.goal_step[0]) == 82


def test_contact_after_separation_and_an_empty_window(ref):
    """two agents that start overlapping, part and meet again: contact_step is the step of the SECOND approach, min_clearance the minimum
    from the first clear step on; an agent whose window holds only itself, and one with an empty window: +inf, no contact"""
    cd = car()
    xs = [0.0, 1.0, 6.0, 9.0, 12.0, 9.0, 7.0, 3.0, 8.0, 11.0]      # the discs sit 1.5 m apart on the axis: clear from 4.33 m on
    path = np.column_stack([np.arange(8.0), np.zeros(8), np.zeros(8)])
    log = HostLog(ref, 4, len(xs), 3, cd.radius, cd.circle_centers)
    got = []
    for s, x in enumerate(xs):
        pool = np.zeros((4, 6))
        pool[1, 0], pool[2, 1], pool[3, 1] = x, 500.0, 900.0
        log.step(np.full((4, 4), 100.0), np.zeros((4, 2)), np.zeros((4, 4, 4)), path, 0, 8, 0, 8, pool, [0, 0, 2, 3], [2, 2, 1, 0], [0, 1, 2, 3])
        got.append(log.rows_f64[s, :, 7].copy())
    got = np.array(got)
    want = np.array([numpy_clearance([0.0, 0.0, 0.0], [[x, 0.0, 0.0]], cd) for x in xs])
    assert np.abs(got[:, 0] - want).max() <= 1e-12 and np.array_equal(got[:, 0], got[:, 1])
    assert want[0] < 0 and want[1] < 0 and want[2] >= 0 and want[7] < 0 and want[8] >= 0      # overlap, apart, a second approach, apart
    contact, minc = outcome_from_clearances(want)
    assert contact == 7
    assert log.contact_step.tolist() == [7, 7, -1, -1]
    assert np.allclose(log.min_clearance[:2], minc, rtol=0, atol=1e-12) and minc == want[7]
    assert np.isinf(got[:, 2:]).all() and (got[:, 2:] > 0).all() and np.isinf(log.min_clearance[2:]).all()
    assert log.flags.tolist() == [1, 1, 1, 1] and log.steps.tolist() == [len(xs)] * 4 and (log.goal_step == -1).all()


def test_overflow_keeps_the_first_rows_and_every_outcome(ref):
    """capacity 3, 5 steps: 3 rows, steps = 5, and the outcomes are those of all 5 steps"""
    cd = car()
    xs = [9.0, 8.0, 7.0, 6.0, 1.0]            # the contact comes in the step after the last row that fits
    path = np.column_stack([np.arange(8.0), np.zeros(8), np.zeros(8)])
    log = HostLog(ref, 2, 3, 3, cd.radius, cd.circle_centers)
    for s, x in enumerate(xs):
        pool = np.zeros((2, 6))
        pool[1, 0] = x
        st = np.array([[7.2, 0.0, 0.01, 0.0], [50.0, 0.0, 3.0, 0.0]]) if s == 4 else np.full((2, 4), 60.0 + s)
        log.step(st, np.zeros((2, 2)), np.zeros((2, 4, 4)), path, 0, 8, 6, 8, pool, 0, 2, [0, 1], iters=s)
    assert log.steps.tolist() == [5, 5]
    assert log.rows_i32[:, :, 5].tolist() == [[0, 0], [1, 1], [2, 2]] and log.rows_f64.shape[0] == 3
    assert np.array_equal(log.rows_f64[:, 0, 0], [60.0, 61.0, 62.0])
    assert log.contact_step.tolist() == [4, 4] and log.goal_step.tolist() == [5, -1]
    assert np.allclose(log.min_clearance, numpy_clearance([0.0, 0.0, 0.0], [[1.0, 0.0, 0.0]], cd), rtol=0, atol=1e-12)


def test_host_build_under_sanitizers(ref, tmp_path):
    """the same source with -fsanitize=address,undefined on a case that walks every branch of the rule (windows that are empty, longer
    than the rule walks or partly outside the pool, agents without a row of their own, failed solves, target indices outside the path, an
    empty path, a capacity smaller than the run): no report, and the numbers of the plain build"""
    exe = str(tmp_path / 'record_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DRECORD_REF_MAIN'] + INC + ['-o', exe, SRC], check=True)
    outp = str(tmp_path / 'out.bin')
    res = subprocess.run([exe, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    n = ref.record_ref_selfcase_size()
    plain = np.zeros(n)
    ref.record_ref_selfcase(plain.ctypes.data)
    san = np.frombuffer(open(outp, 'rb').read(), np.float64)
    assert san.shape == plain.shape and np.allclose(san, plain, rtol=0, atol=1e-12, equal_nan=True)
    P, cap = 7, 4
    rows = plain[:cap * P * 16].reshape(cap, P, 16)
    steps, goal, contact, flags, minc = plain[cap * P * 16:].reshape(P, 5).T
    assert (steps == 9).all() and not (rows == -7.0).all(axis=2).any()
    assert goal.tolist() == [-1, -1, 4, 7, -1, -1, -1]
    assert contact.tolist() == [7, 7] + [contact[2]] + [-1, -1] + [contact[5]] + [-1] and minc[0] == minc[1] == -2.0
    assert np.isinf(minc[3]) and np.isinf(minc[4]) and np.isinf(minc[6]) and np.isfinite(minc[2]) and np.isfinite(minc[5])
    assert np.isnan(rows[1, 1, 6]) and not np.isnan(rows[0, 1, 6])          # agent 1's solve fails in step 1
    assert np.isnan(rows[2, 5, 6]) and np.isnan(rows[3, 5, 6])              # target index beyond / before the path
    assert np.isnan(rows[:, 6, 6]).all()                                    # no path at all


def test_struct_mirrors_match_the_header(ref):
    """_lib.RunLogC against the layout the header's own compiler gives mpcx_run_log and against the field names parsed from the header;
    mpcx_closed_loop is NOT widened (the log travels beside it: mpcx_closed_loop_run_logged), its mirror still has the header's size"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 13)()
    ref.record_ref_layout.restype = None
    ref.record_ref_layout(lay)
    names = [n for n, _ in _lib.RunLogC._fields_]
    assert list(lay)[:12] == [C.sizeof(_lib.RunLogC)] + [getattr(_lib.RunLogC, n).offset for n in names]
    assert lay[12] == C.sizeof(_lib.ClosedLoopC)
    assert C.sizeof(_lib.RunLogC) == 8 + 16 + 7 * 8
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_run_log;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    assert _lib.RUN_LOG_ROW_BYTES == 8 * 8 + 8 * 4 and _lib.RUN_LOG_AGENT_BYTES == 4 * 4 + 8
    assert len(_lib.RUN_LOG_F64) == 8 and len(_lib.RUN_LOG_I32) == 6
    for name in ('mpcx_record_step_batch', 'mpcx_closed_loop_run_logged'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)
    from mpc_for_av_at_intersection_amd.batch import RUN_LOG_DTYPE
    assert RUN_LOG_DTYPE.names == _lib.RUN_LOG_F64 + _lib.RUN_LOG_I32 and RUN_LOG_DTYPE.itemsize == 8 * 8 + 6 * 4


def test_device_kernel_needs_no_lds_and_no_scratch():
    """record_kernel cross-compiled for gfx950 with the Makefile's flags: no LDS, no scratch, no spills, and its rows leave as 16-byte
    stores (at least 4 for the doubles and 2 for the integers)"""
    mk = open(os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('-I$(ROOT)/include', INC[0])
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (.*)$', mk, re.M).group(1).strip()
    src = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'mpcx_record.hip')
    assert os.path.exists(hipcc), 'no hipcc at %s (set HIPCC): the kernel cannot be cross-compiled for this check' % hipcc
    res = subprocess.run([hipcc] + flags.split() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-S', '-o', '-', src],
                         check=True, capture_output=True, text=True)
    assert 'record_kernel' in res.stdout
    use = {k.strip(): int(v) for k, v in re.findall(r'remark: [^\n]*?\s([A-Za-z ]+(?: \[[^\]]*\])?): (\d+) \[-Rpass-analysis', res.stderr)}
    print('record_kernel resources:', use)
    assert use['ScratchSize [bytes/lane]'] == 0 and use['LDS Size [bytes/block]'] == 0
    assert use['VGPRs Spill'] == 0 and use['SGPRs Spill'] == 0 and use['VGPRs'] <= 128
    # the 64 + 32 bytes of a row leave as 16-byte stores: at least 4 + 2 of them (a compiler may split or duplicate, not narrow)
    assert len(re.findall(r'^\s*global_store_dwordx4\b', res.stdout, re.M)) >= 6
