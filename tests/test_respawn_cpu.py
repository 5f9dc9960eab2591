"""Respawn (mpcx_respawn: a departed agent's slot is re-used for the next vehicle of its stream) without a GPU: the host build of
csrc/mpcx_respawn_core.h (tests/respawn_ref/respawn_ref.cpp; respawn_kernel compiles the very same header) against a numpy restatement on
hand-made words, the rule inside the closed loop on the CPU oracle, the sanitizers, the ctypes mirror, the kernel's resource usage and
batch.demand_schedule.  The device side is tests/test_gpu_respawn.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import admit_helpers as AH
from tests import helpers as H
from tests import respawn_helpers as RH

ROOT = RH.ROOT


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return RH.build_ref(tmp_path_factory.mktemp('respawn_ref'))


@pytest.fixture(scope='module')
def admit_ref(tmp_path_factory):
    return AH.build_ref(tmp_path_factory.mktemp('admit_ref'))


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in RH.MUT_F64 + RH.MUT_I32)


@pytest.mark.parametrize('log,speed', [(True, False), (False, False), (True, True), (False, True)])
def test_rule_on_hand_made_words(ref, log, speed):
    """C1.  Nine agents, one per branch (respawn_helpers.hand_made), with and without log words and with prev_len; the host build visiting
    the lanes forwards and backwards and the numpy restatement give identical words.  Driving, waiting, due, finished (served == G), own row
    outside the pool and never-entered agents are untouched; an arrival with vehicles left writes its record, resets every word a first
    step reads and waits max(0, due - clock) steps (30 for a due step of 50 at clock 20, 0 for a past one); the last vehicle writes its
    record and nothing else.  Without a log the log's words are untouched and the record holds -1 / 0 / +inf; without prev_len it is
    untouched.  A second step changes nothing: nobody has arrived."""
    case = RH.hand_made(log, speed)
    before = case.words()
    fwd, bwd, twin = case.copy(), case.copy(), case.copy()
    assert RH.host_step(ref, fwd) == 3 and RH.host_step(ref, bwd, backwards=True) == 3 and RH.numpy_step(twin) == RH.ARRIVE
    after = fwd.words()
    assert _same(after, bwd.words()) and _same(after, twin.words())
    untouched = [q for q in range(case.P) if q not in RH.ARRIVE]
    for k in before:
        assert before[k][untouched].tobytes() == after[k][untouched].tobytes(), k
    assert after['served'].tolist() == [0, 0, 1, 2, 3, 3, 0, 0, 0]
    assert after['wait'].tolist() == [-1, 4, 30, 0, -1, -1, -1, 0, -1] and after['entered'].tolist() == [2, -1, -1, -1, 8, 9, 4, -1, -1]
    for q, g in ((2, 0), (3, 1), (4, 2)):
        want = [case.entered[q], 19, case.steps_driven[q]] + ([case.lsteps[q], case.contact_step[q], case.flags[q]] if log else [-1, -1, 0]) + [case.due[q, g], 0]
        assert after['ep_i32'][q, g].tolist() == want, (q, after['ep_i32'][q, g], want)
        assert after['ep_f64'][q, g].tolist() == [case.min_clearance[q] if log else np.inf, 0.0]
        others = [h for h in range(case.G) if h != g]
        assert (after['ep_i32'][q, others] == -7).all() and (after['ep_f64'][q, others] == -7.0).all()
    assert after['ep_i32'][2, 0, 4] == (41 if log else -1)
    for q in (2, 3):        # reset
        assert np.array_equal(after['state'][q], case.start_state[q]) and not after['applied'][q].any() and not after['u'][q].any()
        assert after['traj_idx'][q] == after['target_ind'][q] == case.start_idx[q]
        assert after['cut_len'][q] == after['iters'][q] == after['steps_driven'][q] == 0
        assert after['prev_len'][q] == (0 if speed else before['prev_len'][q])
        assert after['lsteps'][q] == before['lsteps'][q]            # the cursor keeps counting
        if log:
            assert after['goal_step'][q] == after['contact_step'][q] == -1 and after['flags'][q] == 0 and after['min_clearance'][q] == np.inf
        else:
            for k in ('goal_step', 'contact_step', 'flags', 'min_clearance'):
                assert after[k][q] == before[k][q], k
    for k in before:        # the last vehicle: its record and the count, nothing else
        if k not in ('served', 'ep_i32', 'ep_f64'):
            assert before[k][4].tobytes() == after[k][4].tobytes(), k
    fwd.clock[0] += 1
    assert RH.host_step(ref, fwd) == 0
    assert _same(after, fwd.words())


LONE = {False: [(0, 24, 25), (25, 49, 25), (50, 74, 25)], True: [(0, 22, 23), (23, 45, 23), (46, 68, 23)]}
QUEUE = [[(0, 24, 25), (37, 72, 36), (85, 120, 36)], [(13, 48, 36), (61, 96, 36), (109, 144, 36)]]


@pytest.mark.parametrize('speed', [False, True])
def test_lone_car_on_the_oracle(ref, admit_ref, speed):
    """C2.  The rule inside the closed loop on the CPU oracle (T = 13, v0 = 0): one slot on the stock route (1, 1) from index 600 of 720,
    G = 3, due all 0, gap 0.  Every vehicle is a fresh start, so the three episodes are the same episode one after the other: (entered,
    arrived, driven) = (0, 24, 25), (25, 49, 25), (50, 74, 25) in cut mode and (0, 22, 23), (23, 45, 23), (46, 68, 23) in speed mode.
    (Re-confirmed on the oracle when this test was written: the numbers are what it printed.)"""
    path = H.smoothed_path(1, 1)
    dl = float(np.linalg.norm(path[0, :2] - path[1, :2]))
    loop = RH.RespawnOracleLoop(admit_ref, ref, [path], dl, [600], due=[[0, 0, 0]], gap=0.0, T=13, speed=speed)
    hist = loop.run(120)
    print('lone car, speed=%s: %s in %d steps' % (speed, loop.episodes(0), len(hist)))
    assert len(path) == 720
    assert loop.episodes(0) == LONE[speed]
    assert len(hist) == LONE[speed][-1][1] + 1 and loop.served.tolist() == [3] and loop.wait.tolist() == [-1] and all(loop.done)
    for e, a, d in loop.episodes(0):
        assert d == a - e + 1
    # the slot stays at its last vehicle's final state: the finished slot is not reset
    assert not np.array_equal(loop.state[0], loop.start_state[0])


def test_queue_on_the_oracle(ref, admit_ref):
    """C2.  Two slots on the stock route (1, 1), both from index 600 -- one start pose, one queue --, due = [[0, 10, 60], [5, 20, 30]], gap
    1 m, cut mode.  A vehicle enters once its due step has come, its slot's previous vehicle has arrived AND the other slot's vehicle is 1 m
    clear of the start pose; behind a leader an episode takes 36 steps instead of 25.  The run takes 145 steps, the conflict search hits in
    60 agent-steps.  (Re-confirmed on the oracle when this test was written.)"""
    path = H.smoothed_path(1, 1)
    dl = float(np.linalg.norm(path[0, :2] - path[1, :2]))
    loop = RH.RespawnOracleLoop(admit_ref, ref, [path, path], dl, [600, 600], due=[[0, 10, 60], [5, 20, 30]], gap=1.0, T=13)
    hist = loop.run(200)
    print('queue: %s / %s in %d steps, %d hits' % (loop.episodes(0), loop.episodes(1), len(hist), loop.hits))
    assert [loop.episodes(0), loop.episodes(1)] == QUEUE
    assert len(hist) == 145 and loop.hits == 60
    assert loop.served.tolist() == [3, 3] and (loop.ep_i32[:, :, 6] == loop.due).all()
    for a in range(2):
        for e, arr, d in loop.episodes(a):
            assert d == arr - e + 1
    # never both present at the start pose: in every step at most one of the two entered
    entered = sorted(e for a in range(2) for e, _, _ in loop.episodes(a))
    assert len(set(entered)) == 6 and (loop.ep_i32[:, :, 0] >= loop.due).all()


def test_host_build_under_sanitizers(ref, tmp_path):
    """C3.  the same source with -fsanitize=address,undefined as a stand-alone program on C1's cases, forwards and backwards, two steps
    each: no report, and the words of the plain build"""
    exe = str(tmp_path / 'respawn_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DRESPAWN_REF_MAIN'] + RH.INC + ['-o', exe, RH.SRC], check=True)
    blob, want = b'', b''
    for log, speed in ((True, False), (False, False), (True, True), (False, True)):
        for back in (0, 1):
            c = RH.hand_made(log, speed)
            blob += c.serialise(back, 2)
            for _ in range(2):
                got = RH.host_step(ref, c, backwards=bool(back))
                want += c.blob() + np.int32(got).tobytes()
                c.clock[0] += 1
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    san = open(outp, 'rb').read()
    assert san == want and len(san) > 8000


def test_struct_mirror_matches_the_header(ref):
    """C4.  _lib.RespawnC against the layout the header's own compiler gives mpcx_respawn and the field names parsed from the header; the
    structs respawn travels beside keep their sizes"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 15)()
    ref.respawn_ref_layout(lay)
    names = [n for n, _ in _lib.RespawnC._fields_]
    assert C.sizeof(_lib.RespawnC) == 56 and len(names) == 8
    assert list(lay)[:9] == [C.sizeof(_lib.RespawnC)] + [getattr(_lib.RespawnC, n).offset for n in names]
    assert list(lay)[9:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC), C.sizeof(_lib.SceneC),
                             C.sizeof(_lib.AdmitC)]
    assert (C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC), C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC)) == (24, 80, 32, 16, 40)
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_respawn;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_respawn', 'mpcx_respawn_step_batch'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)
    assert len(_lib.EPISODE_I32) == 7 and len(_lib.EPISODE_F64) == 1


def test_respawn_kernel_needs_no_scratch():
    """C4.  mpcx_respawn.hip cross-compiled for gfx950 with the Makefile's flags: the kernel exists and has no scratch, no spills and no LDS"""
    mk = open(os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('-I$(ROOT)/include', RH.INC[0])
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (.*)$', mk, re.M).group(1).strip()
    src = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'mpcx_respawn.hip')
    assert os.path.exists(hipcc), 'no hipcc at %s (set HIPCC): the kernel cannot be cross-compiled for this check' % hipcc
    res = subprocess.run([hipcc] + flags.split() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-S', '-o', os.devnull, src],
                         check=True, capture_output=True, text=True)
    use, cur = {}, None
    for k, v in re.findall(r'remark:\s+([A-Za-z ]+(?: \[[^\]]*\])?): (\S+) \[-Rpass-analysis', res.stderr):
        if k == 'Function Name':
            cur = use.setdefault(v, {})
        elif cur is not None:
            cur[k.strip()] = int(v) if v.isdigit() else v
    print(use)
    assert len(use) == 1 and any('respawn_kernel' in n for n in use), sorted(use)
    for n, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (n, u)


def test_demand_schedule():
    """C4.  batch.demand_schedule: (B, A, G), deterministic per seed; per approach queue ONE non-decreasing arrival stream dealt to the queue's
    slots in turn (vehicle k to slot k mod n, generation k div n), so every slot's due steps are non-decreasing too; the draws replay as
    cumulative sums of rng.geometric(1 / mean) - 1, instance-major and queue by queue; mean headway 1 gives all zeros"""
    from mpc_for_av_at_intersection_amd.batch import demand_schedule
    routes = []
    for k in range(4):      # four arms with two routes each: routes 2k and 2k + 1 share their first point
        first = np.array([10.0 * k, -30.0, 0.5 * k])
        for m in range(2):
            tail = np.column_stack([10.0 * k + np.arange(1, 6), -30.0 + (m + 1) * np.arange(1, 6), np.full(5, 0.5 * k)])
            routes.append(np.concatenate([first[None], tail]))
    B, A, G = 3, 8, 4
    route_of_agent = np.tile(np.arange(A), (B, 1))
    start = np.zeros((B, A), dtype=np.int64)
    start[2, 1] = 2         # instance 2: slot 1 starts further down its route: a queue of its own
    d = demand_schedule(route_of_agent, routes, start, 6.0, G, seed=3)
    assert d.shape == (B, A, G) and np.issubdtype(d.dtype, np.integer) and (d >= 0).all() and d.max() > 0
    assert np.array_equal(d, demand_schedule(route_of_agent, routes, start, 6.0, G, seed=3))
    assert not np.array_equal(d, demand_schedule(route_of_agent, routes, start, 6.0, G, seed=4))
    rng = np.random.default_rng(3)
    for b in range(B):
        queues = [[0], [1], [2, 3], [4, 5], [6, 7]] if b == 2 else [[0, 1], [2, 3], [4, 5], [6, 7]]
        for qu in queues:
            stream = np.cumsum(rng.geometric(1.0 / 6.0, size=len(qu) * G) - 1)
            assert (np.diff(stream) >= 0).all()
            for k, due in enumerate(stream):
                assert d[b, qu[k % len(qu)], k // len(qu)] == due, (b, qu, k)
    assert (np.diff(d, axis=2) >= 0).all()
    assert not demand_schedule(route_of_agent, routes, start, 1.0, G, seed=3).any()
    assert demand_schedule(route_of_agent, routes, start, 6.0, 1, seed=3).shape == (B, A, 1)
    with pytest.raises(ValueError):
        demand_schedule(route_of_agent, routes, start[:, :4], 6.0, G, seed=3)
    with pytest.raises(ValueError):
        demand_schedule(route_of_agent, routes, start, 6.0, 0, seed=3)
