"""Shared plans (mpcx_intent) without a GPU: the host build of the rule (csrc/mpcx_intent_core.h through tests/intent_ref/intent_ref.cpp;
intent_kernel compiles the very same header) against a numpy restatement on hand-made and seeded words, the two invariants (a constant
plan and T = 1 give the prediction stage's own frames), the same program under the sanitizers, the ctypes mirror, the kernel's resource
use, and the behaviour the stage exists for on the CPU oracle: a car on green is no longer cut in front of a car that is braking for its red
light.  The device side is tests/test_gpu_intent.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import intent_helpers as IH

ROOT = IH.ROOT
# the red-light scene (intent_helpers.red_light_scene) as found on the CPU oracle: start indices of the held and of the green agent, and
# the steps in which the green agent has a conflict (hit_idx >= 0) with the held agent's row, without and with shared plans
RED_LIGHT = dict(held_start=60, green_start=150, tick=50)
RED_LIGHT_HITS = ([0, 2, 8, 9, 10, 11, 12, 13, 14], [0])


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return IH.build_ref(tmp_path_factory.mktemp('intent_ref'))


def _three_ways(ref, w):
    """the host build forwards and backwards and the numpy restatement on copies of w: identical bytes; returns the forward copy and count"""
    fwd, bwd, twin = IH.copy_words(w), IH.copy_words(w), IH.copy_words(w)
    n = [IH.host_rule(ref, fwd), IH.host_rule(ref, bwd, backwards=True), IH.rule_numpy(twin)]
    assert n[0] == n[1] == n[2], n
    for k in ('pred', 'frames'):
        assert fwd[k].tobytes() == bwd[k].tobytes() == twin[k].tobytes(), k
    for k in w:         # nothing else is written
        if k not in ('pred', 'frames') and isinstance(w[k], np.ndarray):
            assert fwd[k].tobytes() == w[k].tobytes(), k
    return fwd, n[0]


def test_rule_on_hand_made_words(ref):
    """I1.  Nine agents in a pool of twelve rows (intent_helpers.hand_made lists what each is there for): every skip reason alone -- share 0,
    done, own row absent, a failed status --, any nonzero share word, a plan that brakes through zero (v is not clamped).  The host build
    visiting the lanes forwards and backwards and the numpy restatement give identical frames and pred, byte for byte; the rows of the
    agents that do not take their plan, and the three rows that are nobody's own, keep every bit; frames is pred_steps or 0."""
    w, takes = IH.hand_made()
    got, n = _three_ways(ref, w)
    assert n == sum(takes) == 4
    S = w['pred'].shape[1]
    assert got['frames'].tolist() == [S if t else 0 for t in takes]
    own = {int(w['obs_skip'][q]): q for q in range(len(takes))}
    for r in range(w['pred'].shape[0]):
        if r in own and takes[own[r]]:
            q = own[r]
            assert not np.array_equal(got['pred'][r], w['pred'][r])
            assert got['pred'][r].tobytes() == IH.plan_roll(w['state'][q], w['u_sol'][q], 0.2, 2.86, IH.CC, S)[0].tobytes(), r
        else:
            assert got['pred'][r].tobytes() == w['pred'][r].tobytes(), r
    # frame k takes column min(k + 1, T - 1): written out for agent 0 (T = 5, 7 frames)
    acc, steer = IH.plan_controls(w['u_sol'][0], S)
    assert acc.tolist() == w['u_sol'][0, 0, [1, 2, 3, 4, 4, 4, 4]].tolist() and steer.tolist() == w['u_sol'][0, 1, [1, 2, 3, 4, 4, 4, 4]].tolist()
    # agent 8 brakes at 5 m/s^2 from 1 m/s: it is predicted to reverse, as the constant prediction of a braking car is
    back = IH.plan_roll(w['state'][8], w['u_sol'][8], 0.2, 2.86, IH.CC, S)[1]
    c, s = np.cos(w['state'][8, 3]), np.sin(w['state'][8, 3])
    along = (back[:, 0] - w['state'][8, 0]) * c + (back[:, 1] - w['state'][8, 1]) * s
    assert along[0] > 0 and along[-1] < along[0]
    # without the retirement words and the scene, agents 2 and 3 take their plans too
    free = IH.copy_words(w); free['done'] = None; free['absent'] = None
    _, n = _three_ways(ref, free)
    assert n == 6


@pytest.mark.parametrize('seed', range(12))
def test_rule_on_seeded_words(ref, seed):
    """I2.  seeded words (1..40 agents, plans of 1..32 columns, 1..64 frames, own rows a random subset of a larger pool, every skip reason,
    with and without done / absent): host build forwards, backwards and numpy identical"""
    _three_ways(ref, IH.random_words(seed))


@pytest.mark.parametrize('T', [1, 2, 5, 20])
def test_constant_plan_is_the_constant_prediction(ref, T):
    """I3.  If every column j >= 1 of a plan equals the applied controls (column 0 is free: it is never read -- except with T = 1, where it
    IS the applied control), the frames are the numpy restatement of predict_row on the pool row, exactly."""
    rng = np.random.default_rng(T)
    P, S = 6, 35
    w = IH.random_words(100 + T)
    state = w['state'][:P]
    applied = np.column_stack([rng.uniform(-2, 2, P), rng.uniform(-0.4, 0.4, P)])      # (acc, steer)
    u = np.repeat(applied[:, :, None], T, axis=2)
    if T > 1:
        u[:, :, 0] = rng.uniform(-1, 1, (P, 2))
    w = IH.words(state=state, u_sol=u, status=np.zeros(P), obs_skip=np.arange(P)[::-1], share=np.ones(P), pred=np.zeros((P, S, 4)), dt=0.2,
                 L=2.86, cc=IH.CC)
    got, n = _three_ways(ref, w)
    assert n == P
    for q in range(P):
        six = np.concatenate([state[q], applied[q]])
        assert got['pred'][P - 1 - q].tobytes() == IH.predict_row_numpy(six, 0.2, 2.86, IH.CC, S)[0].tobytes(), q


def test_horizon_of_one_ignores_nothing_and_equals_the_prediction(ref):
    """I4.  T = 1: the plan is the applied control, whatever it holds -- frames equal predict_row's for random plans"""
    rng = np.random.default_rng(5)
    P, S = 9, 64
    state = np.column_stack([rng.uniform(-30, 30, P), rng.uniform(-30, 30, P), rng.uniform(0, 9, P), rng.uniform(-np.pi, np.pi, P)])
    u = np.stack([rng.uniform(-2, 2, (P, 1)), rng.uniform(-0.4, 0.4, (P, 1))], axis=1)
    w = IH.words(state=state, u_sol=u, status=np.zeros(P), obs_skip=np.arange(P), share=np.ones(P), pred=np.zeros((P, S, 4)), dt=0.2, L=2.86,
                 cc=IH.CC)
    got, _ = _three_ways(ref, w)
    for q in range(P):
        six = np.concatenate([state[q], u[q, :, 0]])
        assert got['pred'][q].tobytes() == IH.predict_row_numpy(six, 0.2, 2.86, IH.CC, S)[0].tobytes(), q


@pytest.mark.parametrize('T', [3, 13, 20])
def test_frames_beyond_and_short_of_the_plan(ref, T):
    """I5.  pred_steps in {1, T - 2, T - 1, T, 35}: shorter than the plan, ending on its last column, one and more beyond it"""
    rng = np.random.default_rng(T)
    P = 5
    state = np.column_stack([rng.uniform(-30, 30, P), rng.uniform(-30, 30, P), rng.uniform(0, 9, P), rng.uniform(-np.pi, np.pi, P)])
    u = np.stack([rng.uniform(-2, 2, (P, T)), rng.uniform(-0.4, 0.4, (P, T))], axis=1)
    for S in (1, T - 2, T - 1, T, 35):
        w = IH.words(state=state, u_sol=u, status=np.zeros(P), obs_skip=np.arange(P), share=np.ones(P), pred=np.zeros((P, S, 4)), dt=0.2,
                     L=2.86, cc=IH.CC)
        got, n = _three_ways(ref, w)
        assert n == P and (got['frames'] == S).all()
        j = np.minimum(np.arange(S) + 1, T - 1)
        for q in range(P):
            assert got['pred'][q].tobytes() == IH.roll(state[q], u[q, 0, j], u[q, 1, j], 0.2, 2.86, IH.CC, S)[0].tobytes(), (S, q)
        if S < 35:      # a shorter horizon is a prefix of a longer one
            long = IH.words(state=state, u_sol=u, status=np.zeros(P), obs_skip=np.arange(P), share=np.ones(P), pred=np.zeros((P, 35, 4)),
                            dt=0.2, L=2.86, cc=IH.CC)
            IH.host_rule(ref, long)
            assert long['pred'][:, :S].tobytes() == got['pred'].tobytes()


def test_host_build_under_sanitizers(ref, tmp_path):
    """I6.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on I1's
    words, forwards and backwards, with and without done / absent, on 120 seeded random cases and on an empty case: no report, and the
    bytes of the numpy restatement"""
    exe = str(tmp_path / 'intent_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DINTENT_REF_MAIN'] + IH.INC + ['-o', exe, IH.SRC], check=True)
    blob, want = b'', b''
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    cases = []
    for back in (0, 1):
        for masks in (True, False):
            w, _ = IH.hand_made()
            if not masks:
                w['done'] = None; w['absent'] = None
            cases.append((w, back))
    cases += [(IH.random_words(seed), seed & 1) for seed in range(120)]
    taken = 0
    for w, back in cases:
        blob += IH.blob(w, back)
        got = IH.rule_numpy(w)
        taken += got
        want += w['frames'].tobytes() + w['pred'].tobytes() + i32(got)
    assert taken > 500
    empty = IH.words(state=np.zeros((0, 4)), u_sol=np.zeros((0, 2, 4)), status=[], obs_skip=[], share=[], pred=np.zeros((0, 5, 4)), dt=0.2,
                     L=2.86, cc=IH.CC)
    blob += IH.blob(empty, 0)
    want += i32(0)
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert open(outp, 'rb').read() == want


def test_struct_mirror_matches_the_header(ref):
    """I7.  _lib.IntentC against the layout the header's own compiler gives mpcx_intent and the field names parsed from the header; the new
    exports are there; every older struct keeps its size"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 18)()
    ref.intent_ref_layout(lay)
    names = [n for n, _ in _lib.IntentC._fields_]
    assert names == ['share', 'frames', 'n_rows', 'reserved']
    assert C.sizeof(_lib.IntentC) == 24
    assert list(lay)[:5] == [C.sizeof(_lib.IntentC)] + [getattr(_lib.IntentC, n).offset for n in names]
    assert list(lay)[5:17] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC),
                               C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC), C.sizeof(_lib.RespawnC), C.sizeof(_lib.RoutesC),
                               C.sizeof(_lib.PrecedenceC), C.sizeof(_lib.SignalsC), C.sizeof(_lib.ActuationC), C.sizeof(_lib.AdviceC)]
    assert list(lay)[6:17] == [24, 80, 32, 16, 40, 56, 64, 24, 88, 80, 40]
    assert lay[17] == C.sizeof(_lib.InteractionParamsC)
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_intent;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_intent', 'mpcx_interaction_batch_intent'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_intent_kernel_needs_no_scratch():
    """I8.  mpcx_intent.hip cross-compiled for gfx950 with the Makefile's flags: exactly its one kernel, no scratch, no spills and no LDS"""
    from tests.test_precedence_cpu import _usage
    use = _usage('mpcx_intent.hip')
    assert len(use) == 1 and 'intent_kernel' in next(iter(use)), sorted(use)
    u = next(iter(use.values()))
    assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, u


def test_no_cut_in_front_of_a_car_braking_for_its_red_light():
    """I9.  Speed mode, stock routes, two_phase_plan(signal_helpers.PLAN) with the clocks at 50: the straight route from the south has red
    for another 50 steps, the straight route from the west has green.  Both cars start at cruise speed, the southern one 60 points into
    its route.  Constant controls predict it straight through the junction until the step in which it brakes, so the car on green has a
    conflict with its row; seen on its plan, it is predicted to stop at its line.  45 steps: nine steps with such a conflict without
    shared plans, one with (step 0, in which no plan exists yet); the worst true clearance of the run is 3.61 m without and 5.47 m with."""
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    from tests import signal_helpers as G
    from tests import speedref_helpers as S
    runs = []
    for share in (None, [True, True]):
        loop = IH.red_light_scene(RED_LIGHT['held_start'], RED_LIGHT['green_start'], share, S.V_REF, two_phase_plan(**G.PLAN), tick=RED_LIGHT['tick'])
        loop.run(45)
        runs.append(loop)
    free, shared = runs
    print('red light: green agent in conflict with the held agent\'s row in steps %s without shared plans, %s with; worst clearance %.3f m / %.3f m'
          % (free.hit_steps[1], shared.hit_steps[1], free.worst_clearance, shared.worst_clearance))
    assert (free.hit_steps[1], shared.hit_steps[1]) == RED_LIGHT_HITS
    assert len(free.hit_steps[1]) >= 1 and len(shared.hit_steps[1]) < len(free.hit_steps[1])
    assert shared.worst_clearance >= free.worst_clearance


def test_stock_instance_measurement():
    """I10.  Measurement only, no threshold: the 8-agent stock instance (instance 0 of synthetic_batch(A = 8, seed = 0), T = 20, cut mode),
    200 steps on the CPU oracle with nobody and with everybody sharing.  Prints the share of agent-steps standing (|v| <= 0.1389 m/s, the
    reference's STOP_SPEED), the mean speed and the worst clearance of both runs; DESIGN.md records them."""
    out = []
    for share in (None, [True] * 8):
        loop = IH.stock_instance(share)
        loop.run(200)
        frac, mean = loop.standing_fraction()
        out.append((frac, mean, loop.worst_clearance, sum(len(h) for h in loop.hit_steps), loop.arrival))
    for name, (frac, mean, clear, hits, arrival) in zip(('constant controls', 'shared plans'), out):
        print('%s: standing %.1f %%, mean speed %.3f m/s, worst clearance %.3f m, %d agent-steps in conflict, arrivals %s'
              % (name, 100 * frac, mean, clear, hits, arrival))
    assert all(np.isfinite(o[0]) and np.isfinite(o[1]) for o in out)
