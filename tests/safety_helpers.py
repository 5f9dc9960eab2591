"""The near-miss log (mpcx_safety: the vehicle nearest to every agent, the first predicted contact, a table of encounters and a conflict
matrix) for the tests: a numpy restatement of the rule, the host build of csrc/mpcx_safety_core.h (tests/safety_ref/safety_ref.cpp) behind
numpy arrays, the hand-made words of tests/test_safety_cpu.py, seeded random scenes, and the rule on a closed loop of the CPU oracle.

The stage decides nothing: a run with it is the run without it plus the words written here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tests import follow_helpers as FH
from tests import signal_helpers as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'safety_ref', 'safety_ref.cpp')
INC = G.INC
MAX_OBS = 16
EV_I32 = ('open', 'last', 'row', 'row_agent', 'path_off', 'partner_path_off', 'traj_idx', 'ttc_frame')
# clearance between the numpy restatement and the host build: both evaluate the same expressions in the same order, sin / cos from libm in
# both, hypot from libm in one and from Python's math module in the other (each within an ulp or two); at distances below 200 m that is
# a few 1e-14 m.  1e-12 leaves a factor of ten.
HOST_TOL = 1e-12


# ---------------------------------------------------------------- the rule, restated
def discs(cc, x, y, yaw):
    """rec_discs: the two disc centres (x, y, x, y) of a car at pose (x, y, yaw)"""
    s, c = math.sin(yaw), math.cos(yaw)
    return (x + (c * cc[0] - s * cc[1]), y + (s * cc[0] + c * cc[1]), x + (c * cc[2] - s * cc[3]), y + (s * cc[2] + c * cc[3]))


def now_of(cc, own6, row6):
    """step 1 for one other row: the smallest distance between a disc of the agent and a disc of the row"""
    e, o = discs(cc, own6[0], own6[1], own6[3]), discs(cc, row6[0], row6[1], row6[3])
    best = math.inf
    for i in (0, 2):
        for j in (0, 2):
            h = math.hypot(e[i] - o[j], e[i + 1] - o[j + 1])
            if h < best:
                best = h
    return best


def contact_of(pred_o, pred_r, lim):
    """step 2 for one other row: the lowest frame k at which a disc of the one touches a disc of the other, -1: none.  pred_*: (S, 4)"""
    d2 = np.full(len(pred_o), np.inf)
    for i in (0, 2):
        for j in (0, 2):
            dx, dy = pred_o[:, i] - pred_r[:, j], pred_o[:, i + 1] - pred_r[:, j + 1]
            d = dx * dx + dy * dy
            d2 = np.where(d < d2, d, d2)
    hit = np.flatnonzero(d2 < lim)
    return int(hit[0]) if len(hit) else -1


def search_numpy(w, q, dists=None):
    """steps 1 and 2 for agent q: (r_now, c_now, r_ttc, k_ttc); dists: a list that receives the per-slot distances of step 1"""
    none = (-1, np.inf, -1, -1)
    n_pool = len(w['obs6'])
    if w.get('done') is not None and w['done'][q]:
        return none
    own = int(w['obs_skip'][q])
    if not 0 <= own < n_pool or (w.get('absent') is not None and w['absent'][own]):
        return none
    slots = FH.others_of(int(w['obs_off'][q]), int(w['obs_cnt'][q]), own, n_pool, w.get('absent'))
    radius = np.float64(w['radius'])
    lim = (np.float64(2.0) * radius) * (np.float64(2.0) * radius)
    r_now, best, r_ttc, k_ttc = -1, np.inf, -1, -1
    for r in slots:
        if r is None:
            continue
        m = now_of(w['cc'], w['obs6'][own], w['obs6'][r])
        if dists is not None:
            dists.append(m)
        if m < best:
            best, r_now = m, r
        k = contact_of(w['pred'][own], w['pred'][r], lim)
        if k >= 0 and (k_ttc < 0 or k < k_ttc):
            k_ttc, r_ttc = k, r
    return r_now, (best - 2.0 * float(radius) if r_now >= 0 else np.inf), r_ttc, k_ttc


def finish_numpy(w, q, found):
    """steps 3 and 4 for agent q"""
    r_now, c_now, r_ttc, k_ttc = found
    w['partner'][q], w['clearance'][q], w['ttc_row'][q], w['ttc_frame'][q] = r_now, c_now, r_ttc, k_ttc
    tick, cap, P = int(w['tick'][q]), int(w['capacity']), len(w['tick'])
    close = r_now >= 0 and c_now < w['near']
    soon = r_ttc >= 0 and 0 <= k_ttc < w['ttc_frames']
    if not close and not soon:
        w['enc_row'][q] = -1
    else:
        p = r_now if close else r_ttc
        if w['enc_row'][q] != p:
            e = int(w['n_events'][q])
            w['n_events'][q] = e + 1
            w['enc_row'][q] = p
            if 0 <= e < cap:
                g = int(w['row_agent'][p])
                g = g if 0 <= g < P else -1
                w['ev_i32'][q, e] = [tick, tick, p, g, w['path_off'][q], w['path_off'][g] if g >= 0 else -1, w['traj_idx'][q], k_ttc]
                w['ev_f64'][q, e] = [c_now, w['state'][q, 2]]
        else:
            e = int(w['n_events'][q]) - 1
            if 0 <= e < cap:
                w['ev_i32'][q, e, 1] = tick
                if k_ttc >= 0 and (w['ev_i32'][q, e, 7] < 0 or k_ttc < w['ev_i32'][q, e, 7]):
                    w['ev_i32'][q, e, 7] = k_ttc
                w['ev_f64'][q, e, 0] = np.fmin(w['ev_f64'][q, e, 0], c_now)
    w['tick'][q] = tick + 1


def rule_numpy(w, backwards=False):
    """one step's stage restated on a dict of numpy arrays (words()), in place on the output words"""
    P = len(w['tick'])
    for q in (range(P - 1, -1, -1) if backwards else range(P)):
        finish_numpy(w, q, search_numpy(w, q))


def margin_numpy(w):
    """the smallest difference between the two smallest step-1 distances of any measured agent (+inf: nobody has two others)"""
    worst = np.inf
    for q in range(len(w['tick'])):
        d = []
        search_numpy(w, q, d)
        d = sorted(x for x in d if x == x)
        if len(d) >= 2:
            worst = min(worst, d[1] - d[0])
    return worst


def class_of(route_off, off):
    hit = np.flatnonzero(np.asarray(route_off) == off) if off >= 0 else []
    return int(hit[0]) if len(hit) else len(route_off)


def summary_numpy(A, route_off, dt, n_events, ev_i32, ev_f64):
    """the conflict matrix: (B, R + 1, R + 1, 3) int64 and (B, R + 1, R + 1, 2) float64"""
    P, cap = ev_i32.shape[0], ev_i32.shape[1]
    B, C_ = P // A, len(route_off) + 1
    out_i, out_f = np.zeros((B, C_, C_, 3), np.int64), np.full((B, C_, C_, 2), np.inf)
    for q in range(P):
        for e in range(min(int(n_events[q]), cap)):
            wd, f = ev_i32[q, e], ev_f64[q, e]
            cell = (q // A, class_of(route_off, wd[4]), class_of(route_off, wd[5]))
            out_i[cell][0] += 1
            out_i[cell][1] += bool(f[0] < 0)
            if wd[7] >= 0:
                out_i[cell][2] += 1
                out_f[cell][1] = min(out_f[cell][1], (np.float64(wd[7]) + 1.0) * np.float64(dt))
            if f[0] < out_f[cell][0]:
                out_f[cell][0] = f[0]
    return out_i, out_f


# ---------------------------------------------------------------- the host build
def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libsafety_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.safety_ref_step.restype = None
    lib.safety_ref_step.argtypes = [C.c_int] * 3 + [C.c_void_p] * 21 + [C.c_double, C.c_int, C.c_int, C.c_int]
    lib.safety_ref_summary.restype = None
    lib.safety_ref_summary.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_double] + [C.c_void_p] * 5
    lib.safety_ref_layout.restype = None
    return lib


I32_KEYS = ('obs_off', 'obs_cnt', 'obs_skip', 'traj_idx', 'path_off')
OPT_KEYS = ('done', 'absent')
STATE_KEYS = ('tick', 'enc_row', 'n_events')
STEP_KEYS = ('partner', 'ttc_row', 'ttc_frame')
OUT_I32 = STEP_KEYS + STATE_KEYS + ('ev_i32',)
OUT_KEYS = OUT_I32 + ('clearance', 'ev_f64')


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes.  The per-step words are allocated as garbage unless
    given; tick and n_events start at 0, enc_row at -1 and the event records as zeros unless given"""
    w = dict(kw)
    for k in I32_KEYS + ('row_agent',):
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    for k in OPT_KEYS:
        w[k] = None if w.get(k) is None else np.ascontiguousarray(w[k], dtype=np.int32)
    for k in ('state', 'obs6', 'pred'):
        w[k] = np.ascontiguousarray(w[k], dtype=np.float64)
    w['cc'] = np.ascontiguousarray(w['cc'], dtype=np.float64).reshape(4)
    P, cap = len(w['traj_idx']), int(w['capacity'])
    assert w['pred'].shape == (len(w['obs6']), w['pred'].shape[1], 4) and len(w['row_agent']) == len(w['obs6'])
    for k in STEP_KEYS:
        w[k] = np.full(P, -7, np.int32) if w.get(k) is None else np.ascontiguousarray(w[k], dtype=np.int32)
    w['clearance'] = np.full(P, np.nan) if w.get('clearance') is None else np.ascontiguousarray(w['clearance'], dtype=np.float64)
    for k, v in (('tick', 0), ('enc_row', -1), ('n_events', 0)):
        w[k] = np.full(P, v, np.int32) if w.get(k) is None else np.ascontiguousarray(w[k], dtype=np.int32)
    w['ev_i32'] = np.zeros((P, cap, 8), np.int32) if w.get('ev_i32') is None else np.ascontiguousarray(w['ev_i32'], dtype=np.int32)
    w['ev_f64'] = np.zeros((P, cap, 2)) if w.get('ev_f64') is None else np.ascontiguousarray(w['ev_f64'], dtype=np.float64)
    w['near'], w['radius'], w['ttc_frames'], w['capacity'] = float(w['near']), float(w['radius']), int(w['ttc_frames']), cap
    return w


copy_words = G.copy_words
geo5 = lambda w: np.array([w['radius']] + list(w['cc']), np.float64)


def host_rule(lib, w, backwards=False):
    """one step's stage through the host build, in place on w (a dict from words())"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    geo = geo5(w)
    lib.safety_ref_step(len(w['traj_idx']), len(w['obs6']), w['pred'].shape[1], geo.ctypes.data, p('obs6'), p('pred'), p('state'), p('obs_off'),
                        p('obs_cnt'), p('obs_skip'), p('traj_idx'), p('path_off'), p('done'), p('absent'), p('row_agent'), p('partner'),
                        p('clearance'), p('ttc_row'), p('ttc_frame'), p('tick'), p('enc_row'), p('n_events'), p('ev_i32'), p('ev_f64'),
                        w['near'], w['ttc_frames'], w['capacity'], int(backwards))


def host_summary(lib, A, route_off, dt, n_events, ev_i32, ev_f64):
    P, cap = ev_i32.shape[0], ev_i32.shape[1]
    ro = np.ascontiguousarray(route_off, dtype=np.int32)
    R = len(ro)
    out_i, out_f = np.zeros((P // A, R + 1, R + 1, 3), np.int64), np.zeros((P // A, R + 1, R + 1, 2))
    n_events, ev_i32, ev_f64 = (np.ascontiguousarray(n_events, dtype=np.int32), np.ascontiguousarray(ev_i32, dtype=np.int32),
                                np.ascontiguousarray(ev_f64, dtype=np.float64))
    lib.safety_ref_summary(P, A, cap, R, ro.ctypes.data, float(dt), n_events.ctypes.data, ev_i32.ctypes.data, ev_f64.ctypes.data,
                           out_i.ctypes.data, out_f.ctypes.data)
    return out_i, out_f


def same_words(a, b, tol):
    """the output words of two runs of the rule: integers exact, clearance and the events' doubles within tol (inf == inf, nan == nan)"""
    for k in OUT_I32:
        assert a[k].tobytes() == b[k].tobytes(), (k, np.argwhere(a[k] != b[k])[:5])
    for k in ('clearance', 'ev_f64'):
        x, y = a[k], b[k]
        fin = np.isfinite(x)
        assert np.array_equal(fin, np.isfinite(y)) and np.array_equal(x[~fin], y[~fin], equal_nan=True), k
        assert len(x[fin]) == 0 or np.abs(x[fin] - y[fin]).max() <= tol, (k, np.abs(x[fin] - y[fin]).max())


def blob(w, frames, backwards, A, route_off, dt):
    """a case of the stand-alone program's input file: the stage runs once per entry of frames = [(obs6, pred), ...] from the words of w"""
    P, n_pool, S = len(w['traj_idx']), len(w['obs6']), w['pred'].shape[1]
    ro = np.ascontiguousarray(route_off, dtype=np.int32)
    b = np.array([P, n_pool, S, w['done'] is not None, w['absent'] is not None, int(backwards), w['ttc_frames'], w['capacity'], len(frames),
                  A, len(ro)], np.int32).tobytes()
    b += np.array([w['near'], dt] + list(geo5(w)), np.float64).tobytes()
    for k in I32_KEYS + OPT_KEYS + ('row_agent',) + STATE_KEYS + ('ev_i32',):
        if w[k] is not None:
            b += w[k].tobytes()
    b += ro.tobytes() + w['state'].tobytes() + w['ev_f64'].tobytes()
    for obs6, pred in frames:
        b += np.ascontiguousarray(obs6, dtype=np.float64).tobytes() + np.ascontiguousarray(pred, dtype=np.float64).tobytes()
    return b


def parse_out(buf, at, w, n_steps, A, R):
    """one case of the stand-alone program's output from byte `at`: (per-step words, final words, matrix or None, the next byte)"""
    P, cap = len(w['traj_idx']), w['capacity']

    def take(dtype, shape):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out = np.frombuffer(buf[at:at + n], dtype=dtype).reshape(shape).copy()
        at += n
        return out
    steps = []
    for _ in range(n_steps):
        steps.append(dict(partner=take(np.int32, (P,)), ttc_row=take(np.int32, (P,)), ttc_frame=take(np.int32, (P,)), clearance=take(np.float64, (P,))))
    fin = dict(tick=take(np.int32, (P,)), enc_row=take(np.int32, (P,)), n_events=take(np.int32, (P,)), ev_i32=take(np.int32, (P, cap, 8)),
               ev_f64=take(np.float64, (P, cap, 2)))
    mat = None
    if A > 0 and P % A == 0:
        B = P // A
        mat = (take(np.int64, (B, R + 1, R + 1, 3)), take(np.float64, (B, R + 1, R + 1, 2)))
    return steps, fin, mat, at


# ---------------------------------------------------------------- hand-made words
HAND_CC = (0.0, 0.0, 2.0, 0.0)      # a rear disc on the reference point, a front disc 2 m ahead; radius 1: discs touch at 2 m
FAR = (50.0, 0)


def frames_of(y, v, S):
    """the predicted discs of a car that heads along x at height y and drifts towards y = 0 at v metres a frame: frame k is at y - v (k + 1)"""
    yk = y - v * (np.arange(S) + 1.0)
    return np.column_stack([np.zeros(S), yk, np.full(S, 2.0), yk])


def hand_pool(agents, S):
    """the pool of hand-made agents, each with a window of its own: its own row first (at the origin, heading along x, standing), then its
    others, each (y, v) or (y, v, 1) = absent: a car beside it at height y > 2 (clearance y - 2 exactly) that drifts towards it at v metres
    a frame, so frame k has d2 = (y - v (k + 1))^2 and the first contact is the lowest k with y - v (k + 1) < 2.
    Returns dict(obs6, pred, absent, obs_off, obs_cnt, obs_skip)"""
    obs6, pred, absent, off, cnt, skip = [], [], [], [], [], []
    for others in agents:
        off.append(len(obs6)); cnt.append(1 + len(others)); skip.append(len(obs6))
        obs6.append((0.0, 0.0, 0.0, 0.0, 0.0, 0.0)); pred.append(frames_of(0.0, 0.0, S)); absent.append(0)
        for o in others:
            obs6.append((0.0, float(o[0]), 0.0, 0.0, 0.0, 0.0)); pred.append(frames_of(float(o[0]), float(o[1]), S)); absent.append(int(len(o) > 2))
    return dict(obs6=np.array(obs6), pred=np.array(pred), absent=absent, obs_off=off, obs_cnt=cnt, obs_skip=skip)


def hand_made(S=35, near=1.5, ttc_frames=5, capacity=2):
    """Hand-made words, one step.  Returns (words, want): want[q] = (slot of the nearest among the agent's others or None, its clearance,
    slot of the first contact or None, its frame at 35 frames) -- a contact beyond the S frames of the call is none."""
    ring = [(20.0 + j, 0) for j in range(15)]       # fifteen standing cars 18 m and more away
    rows = [
        ([], (None, np.inf, None, -1), 0),                              # 0  nobody else
        ([(5, 1)], (0, 3.0, 0, 3), 0),                                  # 1  one other: frames at 4, 3, 2, 1: 2 m does not touch, frame 3 does
        (ring + [(4, 1)], (15, 2.0, 15, 2), 0),                         # 2  exactly 16 others, the nearest and the contact in the last slot
        (ring + [(30, 0), (3, 2)], (0, 18.0, None, -1), 0),             # 3  17 others: the 17th, which touches in frame 0, is ignored
        ([(5, 1)], (None, np.inf, None, -1), 'own_absent'),             # 4  own row absent
        ([(5, 1)], (None, np.inf, None, -1), 'own_low'),                # 5  own row outside the pool, below
        ([(5, 1)], (None, np.inf, None, -1), 'own_high'),               # 6  ... and above
        ([(3, 2, 1), (6, 0)], (1, 4.0, None, -1), 0),                   # 7  an absent other that would be nearest and touch in frame 0
        ([(3, 2)], (None, np.inf, None, -1), 'done'),                   # 8  a done agent
        ([(3, 2)], (0, 1.0, 0, 0), 0),                                  # 9  contact in frame 0: 3 - 2 = 1
        ([(36, 1)], (0, 34.0, 0, 34), 0),                               # 10 contact in the last of 35 frames: 36 - 34 = 2 does not touch, 36 - 35 does
        ([FAR], (0, 48.0, None, -1), 0),                                # 11 no contact
        ([(8, 2), (5, 1)], (1, 3.0, 0, 3), 0),                          # 12 two slots touch in frame 3: the lowest slot; the nearest is the other
        ([(5, 0), (5, 1)], (0, 3.0, 1, 3), 0),                          # 13 two slots equally near: the lowest slot
        ([(3, 2, 1)], (None, np.inf, None, -1), 0),                     # 14 the only other is absent
        ([(3.25, 0)], (0, 1.25, None, -1), 0),                          # 15 near, no contact: an encounter at near = 1.5, none at near = 0
        ([(7, 1)], (0, 5.0, 0, 5), 0),                                  # 16 contact in frame 5: not within ttc_frames = 5
        ([(7, 1.25)], (0, 5.0, 0, 4), 0),                               # 17 contact in frame 4 (7 - 5 1.25 = 0.75): within it
    ]
    pool = hand_pool([r[0] for r in rows], S)
    P, n_pool = len(rows), len(pool['obs6'])
    done = [int(r[2] == 'done') for r in rows]
    for q, r in enumerate(rows):
        if r[2] == 'own_absent':
            pool['absent'][pool['obs_skip'][q]] = 1
        elif r[2] == 'own_low':
            pool['obs_skip'][q] = -1
        elif r[2] == 'own_high':
            pool['obs_skip'][q] = n_pool + 2
    # the rows of agent q's others belong to agent (q + 1) % P, except the last slot of every window: a scripted actor
    owner = np.full(n_pool, -1, np.int32)
    for q in range(P):
        n = pool['obs_cnt'][q] - 1
        owner[pool['obs_off'][q]] = q
        owner[pool['obs_off'][q] + 1:pool['obs_off'][q] + n] = (q + 1) % P
    state = np.zeros((P, 4)); state[:, 2] = 1.0 + 0.5 * np.arange(P)
    w = words(state=state, traj_idx=10 + np.arange(P), path_off=100 * np.arange(P), done=done, row_agent=owner, radius=1.0, cc=HAND_CC,
              near=near, ttc_frames=ttc_frames, capacity=capacity, **pool)
    want = [(r[1][0], r[1][1], r[1][2] if 0 <= r[1][3] < S else None, r[1][3] if 0 <= r[1][3] < S else -1) for r in rows]
    return w, want


def expect_step(w, want):
    """the per-step words from the tuples written down by hand"""
    P = len(want)
    out = dict(partner=np.full(P, -1, np.int32), clearance=np.full(P, np.inf), ttc_row=np.full(P, -1, np.int32), ttc_frame=np.full(P, -1, np.int32))
    for q, (sn, c, st, k) in enumerate(want):
        out['clearance'][q] = c
        if sn is not None:
            out['partner'][q] = w['obs_off'][q] + 1 + sn
        if st is not None:
            out['ttc_row'][q], out['ttc_frame'][q] = w['obs_off'][q] + 1 + st, k
    return out


# the scripted sequence of the encounter state machine: one agent (v = 2.5, traj_idx 7, path_off 300) with two others, A (pool row 1, owned by
# agent 1 whose path_off is 400) and B (pool row 2, a scripted actor), near = 1.5, ttc_frames = 3, 35 frames.  Per step (A, B) as (y, v).
SEQUENCE = [
    (FAR, FAR),                 # 0  nothing
    ((3, 0), FAR),              # 1  A at 1 m: event 0 opens on A
    ((2.5, 1), FAR),            # 2  A at 0.5 m and touching in frame 0: update -- last 2, word 7 = 0, minimum 0.5
    ((3, 0), FAR),              # 3  A at 1 m, no contact: update -- last 3; word 7 and the minimum stay
    ((3, 0), (2.25, 0)),        # 4  B at 0.25 m is nearest: the partner changes, event 1 opens on B
    (FAR, FAR),                 # 5  nothing: closed
    (FAR, (10, 3)),             # 6  B 8 m away touches in frame 2 (7, 4, 1): event 2 opens on B by TTC alone
    (FAR, (10, 1)),             # 7  B touches in frame 8: not within 3 frames -- closed
]
# what a capacity of 8 holds after the sequence: (integer words, doubles) per event
SEQUENCE_EVENTS = [([1, 3, 1, 1, 300, 400, 7, 0], [0.5, 2.5]), ([4, 4, 2, -1, 300, -1, 7, -1], [0.25, 2.5]), ([6, 6, 2, -1, 300, -1, 7, 2], [8.0, 2.5])]
SEQUENCE_ENC = [-1, 1, 1, 1, 2, -1, 2, -1]      # enc_row after every step


def sequence_words(capacity, S=35):
    """the words of the sequence's first step (two agents: agent 1 only owns row 1 and is itself done) and the (obs6, pred) of every step"""
    frames = []
    for a, b in SEQUENCE:
        pool = hand_pool([[a, b]], S)
        frames.append((pool['obs6'], pool['pred']))
    pool = hand_pool([[SEQUENCE[0][0], SEQUENCE[0][1]]], S)
    for k in ('obs_off', 'obs_cnt', 'obs_skip'):
        pool[k] = list(pool[k]) + [0 if k != 'obs_cnt' else 3]
    pool['obs_skip'][1] = 1
    state = np.array([[0, 0, 2.5, 0], [0, 0, 0, 0]], np.float64)
    w = words(state=state, traj_idx=[7, 9], path_off=[300, 400], done=[0, 1], row_agent=[0, 1, -1], radius=1.0, cc=HAND_CC, near=1.5,
              ttc_frames=3, capacity=capacity, **pool)
    return w, frames


def random_words(seed, P=None, S=None):
    """a seeded scene: P agents (1..40 unless given), each with a window of 0..19 others scattered within some twenty metres of it, each row
    with a random pose and a prediction that drifts at a constant velocity with a turning heading, some rows absent, some agents done, some
    own rows absent or outside the pool, some windows that leave the pool; encounter words part-way through a run"""
    rng = np.random.default_rng(seed)
    P = int(rng.integers(1, 41)) if P is None else int(P)
    S = int(rng.choice([1, 2, 7, 35])) if S is None else int(S)
    cc = np.array([0.0, 0.0, 2.7, 0.0]) if seed % 2 else rng.uniform(-1.5, 3.0, 4)
    radius = float(rng.uniform(0.8, 1.6))
    obs6, off, cnt, skip, absent = [], [], [], [], []
    for q in range(P):
        n = int(rng.integers(0, MAX_OBS + 1)) if rng.random() < 0.85 else int(rng.integers(MAX_OBS, MAX_OBS + 4))
        own_at = int(rng.integers(0, n + 1))
        centre = rng.uniform(-60, 60, 2)
        off.append(len(obs6)); cnt.append(n + 1)
        for j in range(n + 1):
            if j == own_at:
                skip.append(len(obs6))
                obs6.append([centre[0], centre[1], rng.uniform(0, 8), rng.uniform(-np.pi, np.pi), 0, 0]); absent.append(int(rng.random() < 0.04))
            else:
                d = rng.uniform(1.0, 25.0) if rng.random() < 0.8 else rng.uniform(0.0, 4.0)
                ang = rng.uniform(-np.pi, np.pi)
                obs6.append([centre[0] + d * np.cos(ang), centre[1] + d * np.sin(ang), rng.uniform(0, 8), rng.uniform(-np.pi, np.pi), 0, 0])
                absent.append(int(rng.random() < 0.1))
    obs6 = np.array(obs6).reshape(-1, 6)
    n_pool = len(obs6)
    # the prediction: the row's discs carried along its heading at its speed, 0.2 s a frame, the heading turning a little
    pred = np.zeros((n_pool, S, 4))
    turn = rng.uniform(-0.05, 0.05, n_pool)
    for r in range(n_pool):
        x, y, v, yaw = obs6[r, :4]
        for k in range(S):
            x, y, yaw = x + v * np.cos(yaw) * 0.2, y + v * np.sin(yaw) * 0.2, yaw + turn[r]
            pred[r, k] = discs(cc, x, y, yaw)
    off, skip = np.array(off), np.array(skip)
    bad = rng.random(P) < 0.05
    off = np.where(bad, rng.integers(-3, n_pool + 3, P), off)           # windows that leave the pool
    skip = np.where(rng.random(P) < 0.04, rng.choice([-1, n_pool, n_pool + 5], P), skip)
    owner = rng.integers(-1, P + 2, n_pool)                             # (some values beyond the agents: read as an actor)
    cap = int(rng.choice([0, 1, 3]))
    n_events = rng.integers(0, 5, P)
    enc = np.where(rng.random(P) < 0.5, -1, rng.integers(0, max(n_pool, 1), P))
    ev_i32 = rng.integers(-1, 30, (P, cap, 8))
    ev_f64 = rng.uniform(-1.0, 5.0, (P, cap, 2))
    return words(state=rng.uniform(-2, 8, (P, 4)), traj_idx=rng.integers(0, 500, P), path_off=rng.integers(0, 5, P) * 700,
                 done=(rng.random(P) < 0.15).astype(np.int32) if seed % 3 else None, absent=absent if seed % 4 else None, row_agent=owner,
                 obs6=obs6, pred=pred, obs_off=off, obs_cnt=cnt, obs_skip=skip, radius=radius, cc=cc,
                 near=float(rng.choice([0.0, 0.5, 3.0])), ttc_frames=int(rng.integers(0, S + 1)), capacity=cap,
                 tick=rng.integers(0, 1000, P), n_events=n_events, enc_row=enc, ev_i32=ev_i32, ev_f64=ev_f64)


# ---------------------------------------------------------------- the rule beside a closed loop of the CPU oracle
def pool_prediction(pool, ip_dt, L, cc, S):
    """moving_obstacles_prediction.py:21-28 for every row (x, y, v, yaw, acc, steer) of a pool, as csrc/mpcx_predict_core.h spells it: (rows,
    S, 4) disc centres"""
    out = np.zeros((len(pool), S, 4))
    for r, (x, y, v, yaw, acc, steer) in enumerate(np.asarray(pool, np.float64)):
        tn = math.tan(steer)
        s, c = math.sin(yaw), math.cos(yaw)
        for k in range(S):
            x, y = x + v * c * ip_dt, y + v * s * ip_dt
            v = v + acc * ip_dt
            yaw = yaw + v / L * tn * ip_dt
            s, c = math.sin(yaw), math.cos(yaw)
            out[r, k] = (x + (c * cc[0] - s * cc[1]), y + (s * cc[0] + c * cc[1]), x + (c * cc[2] - s * cc[3]), y + (s * cc[2] + c * cc[3]))
    return out


class SafetyWatch:
    """the words of the stage for the A agents of one oracle loop (scene_helpers.OracleLoop and its subclasses), advanced with step(),
    which also steps the loop: what safety_kernel sees behind the conflict search of that step"""

    def __init__(self, loop, near, ttc_frames, capacity, S, dt, n_pool):
        self.loop, self.S, self.dt = loop, int(S), float(dt)
        A = loop.A
        owner = np.full(n_pool, -1, np.int32); owner[:A] = np.arange(A)
        offs = np.concatenate([[0], np.cumsum([len(p) for p in loop.paths])[:-1]])
        self.route_off = offs.astype(np.int32)
        self.w = words(state=np.zeros((A, 4)), traj_idx=np.zeros(A), path_off=offs, done=np.zeros(A), absent=np.zeros(n_pool), row_agent=owner,
                       obs6=np.zeros((n_pool, 6)), pred=np.zeros((n_pool, self.S, 4)), obs_off=np.zeros(A), obs_cnt=np.full(A, n_pool),
                       obs_skip=np.arange(A), radius=loop.radius, cc=np.asarray(loop.centers).reshape(4), near=near, ttc_frames=ttc_frames,
                       capacity=capacity)
        self.steps = []

    def step(self):
        """one step of the loop with the stage on the pool that step's conflict search saw and on the nearest indices it left; returns the
        loop's own output"""
        lp, w = self.loop, self.w
        pool, state, done, absent = lp.pool(), lp.state.copy(), list(lp.done), list(lp.absent)
        out = lp.step()
        w['obs6'][:len(pool)] = pool
        w['pred'][:] = pool_prediction(w['obs6'], self.dt, lp.p.L, w['cc'], self.S)
        w['state'][:] = state
        w['traj_idx'][:] = [w['traj_idx'][a] if o is None else o['traj_idx'] for a, o in enumerate(out)]
        w['done'][:] = done
        w['absent'][:lp.A] = absent
        rule_numpy(w)
        self.steps.append({k: w[k].copy() for k in STEP_KEYS + ('clearance',)})
        return out
