"""Admission (mpcx_admit: agents enter the scene on a schedule) without a GPU: the host build of csrc/mpcx_admit_core.h
(tests/admit_ref/admit_ref.cpp; admit_snapshot_kernel and admit_gate_kernel compile the very same header) against a numpy restatement on
hand-made pools, the tie-break, scripted actors, the entry queue of two agents on the CPU oracle, the sanitizers, the ctypes mirror, the
kernels' resource usage and batch.entry_schedule.  The device side is tests/test_gpu_admit.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import admit_helpers as AH
from tests import helpers as H

ROOT = AH.ROOT
WORDS = ('done', 'wait', 'entered', 'absent', 'clock')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return AH.build_ref(tmp_path_factory.mktemp('admit_ref'))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in WORDS)


def test_rule_on_a_hand_made_pool(ref):
    """Six rows (admit_helpers.six_row_pool), gap 1 m: the due agent 1 stands d metres behind the driving agent 0, clearance d - 3.5, so the
    threshold is d = 4.5.  1 mm inside it is held back, 1 mm outside it is admitted -- host build and numpy restatement agree on both sides;
    the nearest row (agent 2's, 0.5 m away, absent) and the departed agent 3 on top of it do not block; agent 2's wait goes 3 -> 2 and
    nothing else of it is written; agent 3 (wait -1) is untouched; agent 4, whose own row lies outside the pool, is due for ever and
    nothing is written for it; admission writes done = 0, absent[own] = 0, wait = -1, entered_step = the clock the step found (7), and
    the clock advances by one per step"""
    for d, want in ((4.499, []), (4.501, [1])):
        case, twin = AH.six_row_pool(d), AH.six_row_pool(d)
        before = case.words()
        got = AH.host_step(ref, case)
        assert AH.numpy_step(twin) == want and got['admitted'] == len(want), (d, got['admitted'])
        after = case.words()
        assert _same(after, twin.words()), (d, after, twin.words())
        assert after['clock'] == 8 and after['wait'].tolist() == [-1, -1 if want else 0, 2, -1, 0, -1]
        assert after['done'].tolist() == [0, 0 if want else 1, 1, 1, 1, 0] and after['absent'].tolist() == [0, 0 if want else 1, 1, 1, 0, 0]
        assert after['entered'].tolist() == [0, 7 if want else -1, -1, 0, -1, 0]
        assert np.array_equal(after['entered'][[0, 2, 3, 4, 5]], before['entered'][[0, 2, 3, 4, 5]])
        # the table: the agents' state rows, bit for bit, and the tags
        assert got['tag'].tolist() == [AH.PRESENT, AH.DUE + 1, AH.GONE, AH.GONE, AH.PRESENT, AH.GONE]
        assert np.array_equal(got['pose'][:5], case.state[[0, 1, 2, 3, 5]][:, [0, 1, 3]]) and np.isnan(got['pose'][5]).all()
    # the clearance the gate judged: the restatement's, and on either side of gap by the millimetre
    for d, side in ((4.499, -1e-3), (4.501, 1e-3)):
        c = AH.six_row_pool(d)
        pose = np.zeros((6, 6)); pose[:, [0, 1, 3]] = c.state[[0, 1, 2, 3, 5, 5]][:, [0, 1, 3]]
        assert abs(AH.SH.clearance(pose, 1, [0, 4], c.centers, c.radius) - (1.0 + side)) < 1e-9
    # the nearest row made present: now it blocks (0.5 m beside: overlapping discs)
    case = AH.six_row_pool(4.501)
    case.absent[2] = 0
    assert AH.host_step(ref, case)['admitted'] == 0 and case.wait.tolist() == [-1, 0, 2, -1, 0, -1]
    # a waiting agent counts down to due and enters in the step after it reads 0
    case = AH.six_row_pool(9.0)
    case.wait[1] = 2
    seen = []
    for _ in range(4):
        AH.host_step(ref, case)
        seen.append((int(case.wait[1]), int(case.done[1]), int(case.entered[1])))
    assert seen == [(1, 1, -1), (0, 1, -1), (-1, 0, 9), (-1, 0, 9)], seen
    assert case.wait[2] == 0 and case.done[2] == 1      # agent 2 is due now, beside the admitted agent 1: held back


@pytest.mark.parametrize('name', sorted(AH.tie_cases()))
def test_tie_break(ref, name):
    """two agents due at one pose with nobody else: only the lower index enters; three with the middle one not due: 0 enters and 2 is
    judged against 0 only (held back at 0's pose, admitted when 0 is far away and only the waiting 1 shares its pose); a due agent that
    is itself held back still has priority over a higher one.  Visiting the agents forwards or backwards gives the same words, and the
    numpy restatement gives them too."""
    case, want = AH.tie_cases()[name]
    fwd, bwd, twin = case.copy(), case.copy(), case.copy()
    assert AH.host_step(ref, fwd, backwards=False)['admitted'] == len(want)
    assert AH.host_step(ref, bwd, backwards=True)['admitted'] == len(want)
    assert AH.numpy_step(twin) == want
    assert _same(fwd.words(), bwd.words()) and _same(fwd.words(), twin.words()), (name, fwd.words(), bwd.words(), twin.words())
    assert [q for q in range(case.P) if case.done[q] and not fwd.done[q]] == want
    # the next step: whoever was held back by a due agent that got in is now held back by a present one
    AH.host_step(ref, fwd); AH.numpy_step(twin)
    assert _same(fwd.words(), twin.words())


def test_actor_poses_are_the_rows_the_traffic_stage_emits(ref):
    """a kinematic T-intersection car and a TAPE car: the pose in the table is bit for bit (x, y, yaw) of the row traffic_get_step emits in
    this step (mpcx_traffic_core.h on the actor's state; for the TAPE car the tape row at its cursor), and the actor's state is unchanged
    by the admission stage.  The ego is held back while the standing car covers its start pose and admitted once that car has driven on."""
    case = AH.actor_case()
    state_before = case.actor_state.copy()
    got = AH.host_step(ref, case)
    assert np.array_equal(case.actor_state, state_before)
    for i in range(2):
        row = np.zeros(6)
        ref.admit_ref_actor_row(case.actors[i:i + 1].ctypes.data, case.actor_state[i].ctypes.data, case.tape.ctypes.data, len(case.tape), row.ctypes.data)
        assert row.tobytes() == got['rows6'][i].tobytes() and got['pose'][case.actor_row[i]].tobytes() == row[[0, 1, 3]].tobytes(), i
    assert got['rows6'][1].tobytes() == case.tape[1 + 2].tobytes()         # tape_off 1, cursor 2
    assert got['rows6'][0, 2] == 0.0 and got['tag'].tolist() == [AH.DUE + 0, AH.PRESENT, AH.PRESENT]
    assert got['admitted'] == 0 and case.done[0] == 1 and case.wait[0] == 0
    twin = AH.actor_case()
    assert AH.numpy_step(twin, got['rows6']) == [] and _same(case.words(), twin.words())
    # the car has driven on (counter beyond its start delay, 20 m down the road): the row it emits carries its speed, and the ego gets in
    for c in (case, twin):
        c.actor_state[0] = [10.0, 3.0, np.pi, 30.0]
    got = AH.host_step(ref, case)
    assert got['rows6'][0, 2] > 6.0 and got['rows6'][0, 0] == 10.0 and np.array_equal(case.actor_state[0], [10.0, 3.0, np.pi, 30.0])
    assert got['admitted'] == 1 and AH.numpy_step(twin, got['rows6']) == [0] and _same(case.words(), twin.words())
    assert case.entered[0] == 1 and case.absent.tolist() == [0, 0, 0]
    # the car hidden (its row absent) on the ego's pose: it does not block
    case = AH.actor_case()
    case.absent[1] = 1
    assert AH.host_step(ref, case)['admitted'] == 1


QUEUE = {  # (gap, routes swapped): (clock at agent 1's entry, clearance at entry, arrivals after steps)
    (0.0, False): (11, 0.0716, (100, 107)),
    (2.0, False): (14, 2.95, (100, 107)),
    (0.0, True): (11, 0.0716, (106, 118)),
    (2.0, True): (14, 2.95, (106, 118)),
}


@pytest.fixture(scope='module')
def queue_runs(ref):
    out = {}
    for (gap, swapped) in QUEUE:
        pair = ((1, 2), (1, 1)) if swapped else ((1, 1), (1, 2))
        paths = [H.smoothed_path(*p) for p in pair]
        dl = float(np.linalg.norm(paths[0][0, :2] - paths[0][1, :2]))
        loop = AH.AdmitOracleLoop(ref, paths, dl, [0, 0], wait=[-1, 0], gap=gap, T=13)
        hist = loop.run(150)
        out[(gap, swapped)] = (loop, hist, paths)
    return out


@pytest.mark.parametrize('gap,swapped', sorted(QUEUE))
def test_entry_queue_on_the_oracle(queue_runs, gap, swapped):
    """The entry queue on the CPU oracle (T = 13, v0 = 0): agents 0 and 1 on the stock routes (1, 1) and (1, 2), both from index 0 -- the
    same pose, (3, -30, pi / 2) --, agent 1 scheduled with wait = 0; every step's decision is the host build of the rule.  Agent 1 is due
    from the first step on and enters when the clock reads 11 (gap 0; clearance at entry 0.0716 m) or 14 (gap 2 m; 2.95 m); they arrive
    in steps (100, 107) of the run, and in (106, 118) with the routes swapped -- the entries are the same.  (Re-confirmed on the oracle
    when this test was written: the numbers above are what it printed.)  The follower has a
    conflict in its first driven step.  Until it enters it is not stepped, and its state is its start pose."""
    loop, hist, paths = queue_runs[(gap, swapped)]
    entry, clearance, arrivals = QUEUE[(gap, swapped)]
    print('gap %.1f swapped %s: entered %s, clearance at entry %s, arrivals %s' % (gap, swapped, loop.entered.tolist(), loop.entry_clearance, loop.arrival))
    assert np.allclose(paths[0][0], [3.0, -30.0, np.pi / 2]) and np.array_equal(paths[0][0], paths[1][0])
    assert loop.entered.tolist() == [0, entry] and loop.wait.tolist() == [-1, -1]
    assert abs(loop.entry_clearance[1] - clearance) < 0.5 * (1e-4 if clearance < 1 else 1e-2), loop.entry_clearance
    assert loop.entry_clearance[1] >= gap
    for s, out in enumerate(hist[:entry]):
        assert out[1] is None and out[0] is not None, s
    assert hist[entry][1] is not None and hist[entry][1]['hit'] >= 0
    # arrivals count the steps of the run; the follower has driven `entry` steps fewer (what retirement's steps_driven holds)
    assert tuple(loop.arrival) == arrivals, loop.arrival
    assert sum(out[1] is not None for out in hist) == arrivals[1] - entry
    assert all(loop.done) and all(loop.absent) and len(hist) == loop.arrival[1]


def test_host_build_under_sanitizers(ref, tmp_path):
    """the same source with -fsanitize=address,undefined (host build only) on the hand-made pools, the tie-break cases and the actor case,
    forwards and backwards, three steps each: no report, and the words of the plain build"""
    exe = str(tmp_path / 'admit_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DADMIT_REF_MAIN'] + AH.INC + ['-o', exe, AH.SRC], check=True)
    cases = [AH.six_row_pool(4.499), AH.six_row_pool(4.501)] + [c for c, _ in AH.tie_cases().values()] + [AH.actor_case()]
    blob, want = b'', []
    for c in cases:
        for back in (0, 1):
            blob += c.serialise(back, 3)
            run = c.copy()
            for _ in range(3):
                got = AH.host_step(ref, run, backwards=bool(back))
                want.append(np.concatenate([run.done, run.wait, run.entered, run.absent, run.clock, [got['admitted']]]).astype(np.int32))
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    san = np.frombuffer(open(outp, 'rb').read(), np.int32)
    assert np.array_equal(san, np.concatenate(want)) and len(san) > 200


def test_struct_mirror_matches_the_header(ref):
    """_lib.AdmitC against the layout the header's own compiler gives mpcx_admit and the field names parsed from the header; the structs
    admission travels beside keep their sizes"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 11)()
    ref.admit_ref_layout(lay)
    names = [n for n, _ in _lib.AdmitC._fields_]
    assert C.sizeof(_lib.AdmitC) == 40
    assert list(lay)[:6] == [C.sizeof(_lib.AdmitC)] + [getattr(_lib.AdmitC, n).offset for n in names]
    assert list(lay)[6:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC), C.sizeof(_lib.SceneC)]
    assert C.sizeof(_lib.ClosedLoopOptsC) == 24 and C.sizeof(_lib.RunLogC) == 8 + 16 + 7 * 8 and C.sizeof(_lib.RetireC) == 32 and C.sizeof(_lib.SceneC) == 16
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_admit;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_admit', 'mpcx_admit_step_batch'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_admit_kernels_need_no_scratch():
    """mpcx_admit.hip cross-compiled for gfx950 with the Makefile's flags: both kernels exist, neither has scratch, spills or static LDS"""
    mk = open(os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('-I$(ROOT)/include', AH.INC[0])
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (.*)$', mk, re.M).group(1).strip()
    src = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'mpcx_admit.hip')
    assert os.path.exists(hipcc), 'no hipcc at %s (set HIPCC): the kernels cannot be cross-compiled for this check' % hipcc
    res = subprocess.run([hipcc] + flags.split() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-S', '-o', os.devnull, src],
                         check=True, capture_output=True, text=True)
    use, cur = {}, None
    for k, v in re.findall(r'remark:\s+([A-Za-z ]+(?: \[[^\]]*\])?): (\S+) \[-Rpass-analysis', res.stderr):
        if k == 'Function Name':
            cur = use.setdefault(v, {})
        elif cur is not None:
            cur[k.strip()] = int(v) if v.isdigit() else v
    print(use)
    assert len(use) == 2 and any('admit_snapshot_kernel' in n for n in use) and any('admit_gate_kernel' in n for n in use), sorted(use)
    for n, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (n, u)


def test_entry_schedule():
    """batch.entry_schedule: deterministic per seed; per approach queue non-decreasing in agent order; the first car of the first queue is
    one draw of rng.geometric(1 / mean) - 1 and the second the sum of two; another seed changes it; mean headway 1 gives all zeros"""
    from mpc_for_av_at_intersection_amd.batch import entry_schedule
    rng = np.random.default_rng(5)
    # four arms with two routes each: routes 2k and 2k + 1 share their first point
    routes = []
    for k in range(4):
        first = np.array([10.0 * k, -30.0, 0.5 * k])
        for m in range(2):
            tail = np.column_stack([10.0 * k + np.arange(1, 6), -30.0 + (m + 1) * np.arange(1, 6), np.full(5, 0.5 * k)])
            routes.append(np.concatenate([first[None], tail]))
    B, A = 5, 8
    route_of_agent = np.tile(np.arange(A), (B, 1))
    route_of_agent[1] = [1, 0, 3, 2, 5, 4, 7, 6]
    start = np.zeros((B, A), dtype=np.int64)
    start[2, 1] = 2         # instance 2: agent 1 starts further down its route: a queue of its own
    w = entry_schedule(route_of_agent, routes, start, 6.0, seed=3)
    assert w.shape == (B, A) and np.issubdtype(w.dtype, np.integer) and (w >= 0).all()
    assert np.array_equal(w, entry_schedule(route_of_agent, routes, start, 6.0, seed=3))
    assert not np.array_equal(w, entry_schedule(route_of_agent, routes, start, 6.0, seed=4))
    for b in range(B):
        for k in range(4):
            if (b, k) != (2, 0):
                assert w[b, 2 * k] <= w[b, 2 * k + 1], (b, k, w[b])
    draws = np.random.default_rng(3).geometric(1.0 / 6.0, size=3) - 1
    assert w[0, 0] == draws[0] and w[0, 1] == draws[0] + draws[1] and w[0, 2] == draws[2]
    # instance-major, queue by first agent index: replay the whole array
    rng = np.random.default_rng(3)
    for b in range(B):
        queues = [[0], [1], [2, 3], [4, 5], [6, 7]] if b == 2 else [[0, 1], [2, 3], [4, 5], [6, 7]]
        for qu in queues:
            assert w[b, qu].tolist() == np.cumsum([rng.geometric(1.0 / 6.0) - 1 for _ in qu]).tolist(), (b, qu)
    assert w.max() > 0
    assert not entry_schedule(route_of_agent, routes, start, 1.0, seed=3).any()
    with pytest.raises(ValueError):
        entry_schedule(route_of_agent, routes, start[:, :4], 6.0, seed=3)
