"""The near-miss log (mpcx_safety) without a GPU: the host build of the rule (csrc/mpcx_safety_core.h through tests/safety_ref/safety_ref.cpp;
safety_kernel and safety_summary_kernel compile the very same header) against a numpy restatement and expectations written down by hand,
the encounter state machine over a scripted sequence, seeded random scenes, the same program under the sanitizers, the ctypes mirror, the
kernels' resource usage, and the rule beside the recorded stock run with its two scripted cars.  The device side is
tests/test_gpu_safety.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import safety_helpers as SF

ROOT = SF.ROOT
# The recorded stock run (T = 13, 82 steps) with the two scripted cars of the stock scenario under near = 0.5 m and ttc = 7.0 s (all 35
# frames of the prediction): the only contact the prediction ever sees once the cars have parted is in frame 34 of step 33, so a shorter
# horizon gives the oracle no event by TTC alone.
STOCK_NEAR, STOCK_TTC_FRAMES = 0.5, 35


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SF.build_ref(tmp_path_factory.mktemp('safety_ref'))


def _three(ref, w):
    """the rule on copies of w: host forwards, host backwards, numpy"""
    fwd, bwd, twin = SF.copy_words(w), SF.copy_words(w), SF.copy_words(w)
    SF.host_rule(ref, fwd); SF.host_rule(ref, bwd, backwards=True); SF.rule_numpy(twin)
    return fwd, bwd, twin


@pytest.mark.parametrize('S,near,ttc_frames', [(35, 1.5, 5), (1, 1.5, 1), (35, 0.0, 5), (35, 1.5, 0), (35, 1.5, 35)])
def test_rule_on_hand_made_words(ref, S, near, ttc_frames):
    """N1.  18 agents, each with a window of its own (safety_helpers.hand_made lists what each is there for): nobody else; 1, 16 and 17
    others; own row absent, below and above the pool; an absent other, and only an absent other; a done agent; contact in frame 0, in
    the last frame, never; two slots in the same frame and two slots equally near; near with no contact; a contact just outside and
    just inside ttc_frames -- with 35 frames and with 1, with near = 0, with ttc_frames = 0 and = pred_steps.  The geometry is exact in
    binary, so the host build forwards and backwards and the numpy restatement give identical bytes, and they are the values written
    down by hand.  An agent is critical iff its clearance is below near or its contact frame below ttc_frames: exactly those open event
    0 on the right partner; nothing else is written."""
    w, want = SF.hand_made(S=S, near=near, ttc_frames=ttc_frames)
    fwd, bwd, twin = _three(ref, w)
    exp = SF.expect_step(w, want)
    for k in SF.OUT_KEYS:
        assert fwd[k].tobytes() == bwd[k].tobytes() == twin[k].tobytes(), k
    for k, v in exp.items():
        assert fwd[k].dtype == v.dtype and fwd[k].tobytes() == v.tobytes(), (k, np.flatnonzero(fwd[k] != v))
    assert sum(k >= 0 for k in exp['ttc_frame']) == (8 if S == 35 else 1) and (exp['partner'] >= 0).sum() == 12
    close = exp['clearance'] < near
    soon = (exp['ttc_frame'] >= 0) & (exp['ttc_frame'] < ttc_frames)
    p = np.where(close, exp['partner'], np.where(soon, exp['ttc_row'], -1))
    assert fwd['enc_row'].tolist() == p.tolist() and fwd['n_events'].tolist() == (p >= 0).astype(int).tolist()
    assert (fwd['tick'] == 1).all()
    if (S, near, ttc_frames) == (35, 1.5, 5):
        assert np.flatnonzero(p >= 0).tolist() == [1, 2, 9, 12, 13, 15, 17]
        # agent 13: nearest is slot 0, but it is critical through the contact of slot 1 in frame 3
        q = 13
        assert fwd['ev_i32'][q, 0].tolist() == [0, 0, w['obs_off'][q] + 2, -1, 1300, -1, 23, 3] and fwd['ev_f64'][q, 0].tolist() == [3.0, 7.5]
        # agent 12: slot 0 of two belongs to agent 13
        assert fwd['ev_i32'][12, 0].tolist() == [0, 0, w['obs_off'][12] + 1, 13, 1200, 1300, 22, 3]
    if near == 0.0:
        assert not close.any() and p[15] == -1
    if ttc_frames == 0:
        assert np.flatnonzero(p >= 0).tolist() == [9, 15]
    for k in w:         # nothing else is written
        if k not in SF.OUT_KEYS and isinstance(w[k], np.ndarray):
            assert fwd[k].tobytes() == w[k].tobytes(), k
    # without the retirement words agent 8 is agent 9's twin; without the scene's words the absent rows are seen
    free = SF.copy_words(w); free['done'] = None
    SF.host_rule(ref, free)
    assert free['partner'][8] == w['obs_off'][8] + 1 and free['clearance'][8] == 1.0 and free['ttc_frame'][8] == 0
    seen = SF.copy_words(w); seen['absent'] = None
    SF.host_rule(ref, seen)
    assert seen['partner'][7] == w['obs_off'][7] + 1 and seen['clearance'][7] == 1.0 and seen['partner'][4] == w['obs_off'][4] + 1


@pytest.mark.parametrize('capacity', [8, 1, 0])
def test_encounter_state_machine(ref, capacity):
    """N2.  The scripted sequence of safety_helpers.SEQUENCE, eight steps: open on A; update (last tick, the smaller contact frame, the
    minimum clearance); update that keeps both; the partner changes to B: a second event; not critical: closed; B again, by TTC alone: a
    third event; a contact beyond ttc_frames: closed.  Capacity 8 holds the three records written down by hand; capacity 1 holds the
    first and counts three; capacity 0 counts three and stores nothing.  enc_row after every step is as written down, the tick is 8."""
    w, frames = SF.sequence_words(capacity)
    host, twin = SF.copy_words(w), SF.copy_words(w)
    for s, (obs6, pred) in enumerate(frames):
        for x, run in ((host, lambda x: SF.host_rule(ref, x, backwards=s & 1)), (twin, SF.rule_numpy)):
            x['obs6'], x['pred'] = np.ascontiguousarray(obs6), np.ascontiguousarray(pred)
            run(x)
            assert x['enc_row'].tolist() == [SF.SEQUENCE_ENC[s], -1], s
    for k in SF.OUT_KEYS:
        assert host[k].tobytes() == twin[k].tobytes(), k
    assert host['tick'].tolist() == [8, 8] and host['n_events'].tolist() == [3, 0]
    for e, (wi, wf) in enumerate(SF.SEQUENCE_EVENTS[:capacity]):
        assert host['ev_i32'][0, e].tolist() == wi and host['ev_f64'][0, e].tolist() == wf, e
    assert not host['ev_i32'][0, 3:].any() and not host['ev_i32'][1].any()


def test_numpy_rule_equals_the_host_build_on_seeded_scenes(ref):
    """N3.  60 seeded scenes (1..40 agents, 0..19 others each, 1 to 35 frames, absent rows, done agents, own rows absent or outside the
    pool, windows that leave the pool, row_agent values beyond the agents, encounter words part-way through a run, capacity 0, 1 and 3).
    The two smallest distances of every agent differ by more than 1e-6 (asserted), so `partner` cannot hinge on an ulp; then every
    integer word is identical, clearance and the events' doubles agree within 1e-12, and visiting the agents backwards changes no byte."""
    seen = dict(partner=0, contact=0, opened=0, updated=0)
    for seed in range(60):
        w = SF.random_words(seed)
        assert SF.margin_numpy(w) > 1e-6, seed
        fwd, bwd, twin = _three(ref, w)
        for k in SF.OUT_KEYS:
            assert fwd[k].tobytes() == bwd[k].tobytes(), (seed, k)
        SF.same_words(fwd, twin, SF.HOST_TOL)
        seen['partner'] += int((fwd['partner'] >= 0).sum()); seen['contact'] += int((fwd['ttc_frame'] >= 0).sum())
        seen['opened'] += int((fwd['n_events'] > w['n_events']).sum())
        seen['updated'] += int(((fwd['n_events'] == w['n_events']) & (fwd['enc_row'] >= 0)).sum())
    assert seen['partner'] > 500 and seen['contact'] > 100 and seen['opened'] > 50, seen


def _matrix_table():
    """a hand-made event table for the conflict matrix: B = 2, A = 2, capacity 3, routes at offsets 0, 700 and 700 again (the lowest
    of equals is the class)"""
    n_events = np.array([3, 5, 0, 1], np.int32)         # agent 1 opened five, three stored
    ev_i32 = np.zeros((4, 3, 8), np.int32); ev_f64 = np.zeros((4, 3, 2))
    ev = lambda q, e, po, pp, k, c: (ev_i32.__setitem__((q, e), [0, 0, 0, 0, po, pp, 0, k]), ev_f64.__setitem__((q, e), [c, 1.0]))
    ev(0, 0, 0, 700, 4, 0.25)       # (0, 1): predicted in frame 4
    ev(0, 1, 0, 700, 9, -0.5)       # (0, 1): a contact, predicted in frame 9
    ev(0, 2, 0, -1, -1, 0.125)      # (0, R): an actor partner
    ev(1, 0, 700, 0, -1, np.nan)    # (1, 0): a clearance that is no number
    ev(1, 1, 1400, 0, 0, 0.375)     # (R, 0): an unknown offset
    ev(1, 2, 700, 0, -1, 0.0625)    # (1, 0)
    ev(2, 0, 0, 0, 3, -9.0)         # not stored: n_events is 0
    ev(3, 0, 700, 700, 34, -0.25)   # instance 1, (1, 1)
    return n_events, ev_i32, ev_f64, np.array([0, 700, 700], np.int32)


def test_conflict_matrix_on_a_hand_made_table(ref):
    """N4.  The conflict matrix of the host build and of the numpy restatement on a hand-made event table with an actor partner (class R),
    an unknown offset (class R), a NaN clearance (counted, skipped in the minimum), a record beyond n_events (ignored), an agent that
    opened more events than are stored, and two routes with the same offset (the lowest is the class): the cells written down by hand"""
    n_events, ev_i32, ev_f64, routes = _matrix_table()
    hi, hf = SF.host_summary(ref, 2, routes, 0.2, n_events, ev_i32, ev_f64)
    ni, nf = SF.summary_numpy(2, routes, 0.2, n_events, ev_i32, ev_f64)
    assert hi.tobytes() == ni.tobytes() and hf.tobytes() == nf.tobytes()
    assert hi.shape == (2, 4, 4, 3) and hi.sum(axis=(1, 2)).tolist() == [[6, 1, 3], [1, 1, 1]]
    assert hi[0, 0, 1].tolist() == [2, 1, 2] and hf[0, 0, 1].tolist() == [-0.5, 5 * 0.2]
    assert hi[0, 0, 3].tolist() == [1, 0, 0] and hf[0, 0, 3].tolist() == [0.125, np.inf]
    assert hi[0, 1, 0].tolist() == [2, 0, 0] and hf[0, 1, 0].tolist() == [0.0625, np.inf]
    assert hi[0, 3, 0].tolist() == [1, 0, 1] and hf[0, 3, 0].tolist() == [0.375, 0.2]
    assert hi[1, 1, 1].tolist() == [1, 1, 1] and hf[1, 1, 1].tolist() == [-0.25, 35 * 0.2]
    assert not hi[:, 2].any() and not hi[:, :, 2].any() and np.isinf(hf[0, 0, 0]).all()
    # no routes at all: one cell per instance
    hi0, hf0 = SF.host_summary(ref, 2, np.zeros(0, np.int32), 0.2, n_events, ev_i32, ev_f64)
    assert hi0.reshape(2, 3).tolist() == [[6, 1, 3], [1, 1, 1]] and hf0.reshape(2, 2).tolist() == [[-0.5, 0.2], [-0.25, 7.0]]


def test_host_build_under_sanitizers(ref, tmp_path):
    """N5.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on N1's
    words with and without the optional words, forwards and backwards, on N2's sequence at every capacity, on the 60 scenes of N3 and on an
    empty case, each followed by the conflict matrix of its events: no report; the integer words are those of the numpy restatement, the
    doubles within 1e-12"""
    exe = str(tmp_path / 'safety_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DSAFETY_REF_MAIN'] + SF.INC + ['-o', exe, SF.SRC], check=True)
    cases = []          # (words, frames, backwards, A, route_off)
    for S, near, tf in ((35, 1.5, 5), (1, 1.5, 1), (35, 0.0, 0)):
        for back in (0, 1):
            for drop in ((), ('done',), ('absent',)):
                w, _ = SF.hand_made(S=S, near=near, ttc_frames=tf)
                for k in drop:
                    w[k] = None
                cases.append((w, [(w['obs6'], w['pred'])], back, 6, 100 * np.arange(0, 18, 2)))
    for cap in (8, 1, 0):
        w, frames = SF.sequence_words(cap)
        cases.append((w, frames, 0, 2, [300, 400]))
    for seed in range(60):
        w = SF.random_words(seed)
        cases.append((w, [(w['obs6'], w['pred'])], seed & 1, 1, [0, 700, 1400]))
    w = SF.random_words(3, P=4)
    empty = SF.words(**{k: (v[:0] if isinstance(v, np.ndarray) and k in SF.I32_KEYS + SF.OUT_KEYS + ('state', 'done') else v) for k, v in w.items()})
    cases.append((empty, [(empty['obs6'], empty['pred'])], 0, 1, []))
    blob = b''.join(SF.blob(w, frames, back, A, ro, 0.2) for w, frames, back, A, ro in cases)
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    buf, at = open(outp, 'rb').read(), 0
    for w, frames, back, A, ro in cases:
        steps, fin, mat, at = SF.parse_out(buf, at, w, len(frames), A, len(ro))
        for s, (obs6, pred) in enumerate(frames):
            w['obs6'], w['pred'] = np.ascontiguousarray(obs6), np.ascontiguousarray(pred)
            SF.rule_numpy(w)
            SF.same_words(dict(w, **steps[s]), dict(w), SF.HOST_TOL)
        SF.same_words(dict(w, **fin), dict(w), SF.HOST_TOL)
        ni, nf = SF.summary_numpy(A, np.asarray(ro, np.int32), 0.2, fin['n_events'], fin['ev_i32'], fin['ev_f64'])
        assert mat[0].tobytes() == ni.tobytes() and mat[1].tobytes() == nf.tobytes()
    assert at == len(buf)


def test_struct_mirror_matches_the_header(ref):
    """N6.  _lib.SafetyC against the layout the header's own compiler gives mpcx_safety and the field names parsed from the header; the
    new exports are there and declared; the stage is no row of the stage table and adds no entry point"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 17)()
    ref.safety_ref_layout(lay)
    names = [n for n, _ in _lib.SafetyC._fields_]
    assert names == ['partner', 'clearance', 'ttc_row', 'ttc_frame', 'tick', 'enc_row', 'n_events', 'ev_i32', 'ev_f64', 'row_agent', 'near',
                     'ttc_frames', 'capacity', 'n_rows', 'n_pool', 'reserved']
    assert C.sizeof(_lib.SafetyC) == 112
    assert list(lay) == [C.sizeof(_lib.SafetyC)] + [getattr(_lib.SafetyC, n).offset for n in names]
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_safety;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_set_safety', 'mpcx_safety_step_batch', 'mpcx_safety_summary'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)
    assert 'safety' not in _lib.STAGE_KEYS and len(_lib.STAGES) == 13 and len(_lib.LOOP_ENTRY_POINTS) == 14
    assert len(_lib.SAFETY_I32) == 8 and _lib.SAFETY_I32 == SF.EV_I32 and len(_lib.SAFETY_F64) == 2


def test_safety_kernels_need_no_scratch():
    """N7.  mpcx_safety.hip cross-compiled for gfx950 with the Makefile's flags: exactly its two kernels, no scratch, no spills and no LDS"""
    from tests.test_precedence_cpu import _usage
    use = _usage('mpcx_safety.hip')
    assert len(use) == 2 and sorted('summary' in n for n in use) == [False, True], sorted(use)
    for name, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (name, u)


def stock_scene_words(capacity=8):
    """the recorded stock run (closedloop.npz, T = 13) with the two scripted cars of the stock scenario, as the words of the stage per step:
    (words, [(obs6, pred, state, traj_idx)] per step)"""
    from tests.test_runlog_cpu import car, golden_vehicles, stock_run
    cd = car()
    run = stock_run('closedloop.npz', 13, 1)
    objs = [o for n, o, _ in golden_vehicles() if n.startswith('stock')]
    cars = np.stack([o.tape(run['n']) for o in objs], axis=1)
    cc = np.asarray(cd.circle_centers, np.float64).reshape(4)
    steps = []
    for i in range(run['n']):
        prev = run['ctrl'][i - 1] if i else np.zeros(2)
        pool = np.concatenate([np.concatenate([run['pre'][i], [prev[1], prev[0]]])[None], cars[i]])
        steps.append((pool, SF.pool_prediction(pool, 0.2, cd.distance_back_to_front_wheel, cc, 35), run['pre'][i][None], [run['tidx'][i]]))
    w = SF.words(state=steps[0][2], traj_idx=[0], path_off=[0], done=None, absent=None, row_agent=[0, -1, -1], obs6=steps[0][0], pred=steps[0][1],
                 obs_off=[0], obs_cnt=[3], obs_skip=[0], radius=float(cd.radius), cc=cc, near=STOCK_NEAR, ttc_frames=STOCK_TTC_FRAMES,
                 capacity=capacity)
    return w, steps


# (open, last, pool row, smallest contact frame) of the ego's events over the 82 steps, and the minimum clearance of each to 1e-9
STOCK_EVENTS = [(0, 24, 2, 0), (33, 33, 2, 34)]
STOCK_MIN_CLEARANCE = [-2.82842712474619, 11.573791596665066]


def test_stock_scene_with_its_two_scripted_cars(ref):
    """N8.  The stock scenario with its two scripted cars on the CPU: the recorded run of the oracle's goldens (82 steps, T = 13) and the
    cars' own tapes, the prediction restated from csrc/mpcx_predict_core.h, near = 0.5 m, ttc = 7 s (35 frames).  The second car spawns ON
    the ego's start pose (the header of mpcx_record_core.h), so step 0 opens a contact event on pool row 2 that lasts the 25 steps the
    discs overlap (minimum -2 radius); in step 33 the same car, 11.6 m away by then, is predicted to touch the ego in frame 34: an event
    opened by TTC alone.  Recorded counts: 2 events, 1 contact event, 1 event by TTC alone.  Host build and numpy agree step by step; the
    clearance column is test_runlog_cpu's clearance of the run."""
    w, steps = stock_scene_words()
    host, twin = SF.copy_words(w), SF.copy_words(w)
    clr = []
    for obs6, pred, state, ti in steps:
        for x in (host, twin):
            x['obs6'], x['pred'], x['state'] = np.ascontiguousarray(obs6), np.ascontiguousarray(pred), np.ascontiguousarray(state)
            x['traj_idx'] = np.asarray(ti, np.int32)
        SF.host_rule(ref, host); SF.rule_numpy(twin)
        SF.same_words(host, twin, SF.HOST_TOL)
        clr.append(host['clearance'][0])
    n = int(host['n_events'][0])
    ev = [(int(a[0]), int(a[1]), int(a[2]), int(a[7])) for a in host['ev_i32'][0, :n]]
    print('stock scene: events (open, last, row, ttc word) %s, min clearance %s' % (ev, host['ev_f64'][0, :n, 0].tolist()))
    contact = [e for e, f in zip(ev, host['ev_f64'][0, :n, 0]) if f < 0]
    by_ttc = [e for e, f in zip(ev, host['ev_f64'][0, :n, 0]) if f >= STOCK_NEAR]
    assert len(contact) >= 1 and len(by_ttc) >= 1
    assert contact[0][0] == 0 and contact[0][2] == 2 and abs(host['ev_f64'][0, 0, 0] + 2 * w['radius']) <= 1e-12
    assert ev == STOCK_EVENTS
    assert np.abs(host['ev_f64'][0, :n, 0] - STOCK_MIN_CLEARANCE).max() <= 1e-9 and (len(contact), len(by_ttc)) == (1, 1)
    assert int(host['tick'][0]) == len(steps) == 82
    clr = np.array(clr)
    assert (clr[:25] < 0).all() and clr[25:].min() > 1.0          # test_runlog_cpu: below 0 for the car's start delay + 5 steps
