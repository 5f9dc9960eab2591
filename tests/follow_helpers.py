"""Car following (mpcx_following: an agent keeps a standstill distance and a time gap to the car ahead of it on its own path) for the tests: a
numpy restatement of the rule, the host build of csrc/mpcx_follow_core.h (tests/follow_ref/follow_ref.cpp) behind numpy arrays, the hand-made
words of tests/test_follow_cpu.py, seeded random scenes, and the closed loop of several egos on the CPU oracle under the rule
(FollowOracleLoop, a subclass of signal_helpers.SignalOracleLoop).

The rule lowers the cut length (the stop index in speed mode) to a stop point behind the leader and, in speed mode, caps row 2 of the
agent's xref: a step with following is the step without it with min(cut, s) in place of cut and minimum(speed profile, cap) in place of
the speed profile for every agent with a leader."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle_py as orc
from tests import scene_helpers as SH
from tests import signal_helpers as G
from tests import speedref_helpers as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'follow_ref', 'follow_ref.cpp')
INC = G.INC
MAX_OBS = 16
STEPS_MAX = 1 << 30
WRAP_TURNS = 32
TWO_PI = 6.283185307179586
PAR = ('standstill', 'time_gap', 'brake', 'v_min', 'lateral', 'heading')

# the parameters the behaviour tests run with: IntersectionBatch.follow's defaults (reach: 40 m of the stock paths' 0.083 m points)
FOLLOW = dict(standstill=6.0, time_gap=1.0, brake=3.0, v_min=0.5, lateral=1.5, heading=0.8, reach=482)


# ---------------------------------------------------------------- the rule, restated
def others_of(off, cnt, own, n_pool, absent=None):
    """the slots of an agent's window: the rows other than its own, in row order, the first 16; None where a row is outside the pool or absent"""
    rows = [r for r in range(off, off + max(cnt, 0)) if r != own][:MAX_OBS]
    return [r if 0 <= r < n_pool and not (absent is not None and absent[r]) else None for r in rows]


def project(path, ti, last, x, y):
    """step 1: (d2, k*) of the point of path[ti .. last] nearest to (x, y), the lowest k of equals"""
    dx, dy = path[ti:last + 1, 0] - np.float64(x), path[ti:last + 1, 1] - np.float64(y)
    d2 = dx * dx + dy * dy
    if not (d2 < np.inf).any():
        return np.inf, ti
    k = int(np.argmin(np.where(np.isnan(d2), np.inf, d2)))          # (argmin returns the first of equals)
    return np.float64(d2[k]), ti + k


def heads_along(yaw_path, yaw_row, heading):
    w = np.float64(yaw_path) - np.float64(yaw_row)
    if not abs(w) <= np.float64(WRAP_TURNS + 1) * np.float64(TWO_PI):
        return False
    for _ in range(WRAP_TURNS + 1):
        if w > np.pi:
            w = w - np.float64(TWO_PI)
    for _ in range(WRAP_TURNS + 1):
        if w < -np.pi:
            w = w + np.float64(TWO_PI)
    return bool(abs(w) <= heading)


def leader_of(path, ti, rows6, slots, par, reach):
    """steps 1 - 3 for one agent on its own path (L, 3): (pool row, k*, v of the row) or None.  rows6: the pool; slots: others_of()"""
    if not 0 <= ti < len(path):
        return None
    last = min(ti + int(reach), len(path) - 1)
    best = None
    for r in slots:
        if r is None:
            continue
        d2, k = project(path, ti, last, rows6[r, 0], rows6[r, 1])
        if k <= ti or not d2 <= np.float64(par['lateral']) * np.float64(par['lateral']):
            continue
        if not heads_along(path[k, 2], rows6[r, 3], par['heading']):
            continue
        if best is None or k < best[1]:
            best = (r, k, float(rows6[r, 2]))
    return best


def stop_and_cap(ti, k, v_l, v_ego, dl, speed, par):
    """steps 3 - 5 for an agent with a leader at k: (gap, stop point s, cap)"""
    f = {n: np.float64(par[n]) for n in PAR}
    gap = np.float64(k - ti) * np.float64(dl)
    vl, v = max(np.float64(v_l), np.float64(0.0)), max(np.float64(v_ego), np.float64(0.0))
    need = f['standstill'] if speed else f['standstill'] + f['time_gap'] * v
    nd = np.ceil(need / np.float64(dl))
    n = int(nd) if nd < STEPS_MAX else STEPS_MAX
    s = max(k - n, ti + 1)
    room = max(gap - f['standstill'], np.float64(0.0))
    bt = f['brake'] * f['time_gap']
    vs = np.sqrt((bt * bt + vl * vl) + (np.float64(2.0) * f['brake']) * room) - bt
    return float(gap), int(s), float(max(vs, f['v_min']))


def rule_numpy(w):
    """the search stage restated on a dict of numpy arrays (words()), in place on leader, gap, cap and cut_len; returns the number of leaders"""
    got = 0
    n_pool = len(w['obs6'])
    for q in range(len(w['traj_idx'])):
        w['leader'][q], w['gap'][q], w['cap'][q] = -1, -1.0, 0.0
        if w.get('done') is not None and w['done'][q]:
            continue
        own = -1 if w.get('obs_skip') is None else int(w['obs_skip'][q])
        ti, ln, off = int(w['traj_idx'][q]), int(w['path_len'][q]), int(w['path_off'][q])
        if not 0 <= ti < ln:
            continue
        slots = others_of(int(w['obs_off'][q]), int(w['obs_cnt'][q]), own, n_pool, w.get('absent'))
        best = leader_of(w['path'][off:off + ln], ti, w['obs6'], slots, w, w['reach'])
        if best is None:
            continue
        gap, s, cap = stop_and_cap(ti, best[1], best[2], w['state'][q, 2], w['dl'], w['speed'], w)
        w['leader'][q], w['gap'][q], w['cap'][q] = best[0], gap, cap
        w['cut_len'][q] = min(int(w['cut_len'][q]), s)
        got += 1
    return got


def clamp_numpy(w):
    """step 6 on w['xref'] (P, 4, W) from w['cap']"""
    for q in range(len(w['cap'])):
        if w.get('done') is not None and w['done'][q]:
            continue
        if w['cap'][q] > 0.0:
            w['xref'][q, 2] = np.fmin(w['xref'][q, 2], w['cap'][q])


# ---------------------------------------------------------------- the host build
def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libfollow_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.follow_ref_step.restype = C.c_int
    lib.follow_ref_step.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 16 + [C.c_int, C.c_int]
    lib.follow_ref_clamp.restype = None
    lib.follow_ref_clamp.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.follow_ref_layout.restype = None
    return lib


I32_KEYS = ('path_off', 'path_len', 'traj_idx', 'cut_len', 'obs_off', 'obs_cnt')
OPT_KEYS = ('done', 'obs_skip', 'absent')
F64_KEYS = ('state', 'path', 'obs6')


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes; the outputs are allocated (garbage) unless given"""
    w = dict(kw)
    for k in I32_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    for k in OPT_KEYS:
        w[k] = None if w.get(k) is None else np.ascontiguousarray(w[k], dtype=np.int32)
    for k in F64_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.float64)
    P = len(w['traj_idx'])
    w['leader'] = np.full(P, -7, np.int32) if w.get('leader') is None else np.ascontiguousarray(w['leader'], dtype=np.int32)
    for k in ('gap', 'cap'):
        w[k] = np.full(P, np.nan) if w.get(k) is None else np.ascontiguousarray(w[k], dtype=np.float64)
    if w.get('xref') is not None:
        w['xref'] = np.ascontiguousarray(w['xref'], dtype=np.float64)
    w['speed'], w['reach'] = int(w['speed']), int(w['reach'])
    return w


copy_words = G.copy_words
par6 = lambda w: np.array([w[n] for n in PAR], np.float64)


def host_rule(lib, w, backwards=False):
    """the search stage through the host build, in place on w (a dict from words()); returns the number of leaders"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    par = par6(w)
    return lib.follow_ref_step(len(w['traj_idx']), len(w['obs6']), float(w['dl']), w['speed'], p('state'), p('path'), p('path_off'), p('path_len'),
                               p('traj_idx'), p('cut_len'), p('done'), p('obs6'), p('obs_off'), p('obs_cnt'), p('obs_skip'), p('absent'),
                               p('leader'), p('gap'), p('cap'), par.ctypes.data, w['reach'], int(backwards))


def host_clamp(lib, w, backwards=False):
    P, _, W = w['xref'].shape
    lib.follow_ref_clamp(P, W, None if w['done'] is None else w['done'].ctypes.data, w['cap'].ctypes.data, w['xref'].ctypes.data, int(backwards))


def blob(w, backwards):
    """a case of the stand-alone program's input file"""
    P, W = len(w['traj_idx']), (w['xref'].shape[2] if w.get('xref') is not None else 0)
    b = np.array([P, len(w['obs6']), len(w['path']), W, w['done'] is not None, w['obs_skip'] is not None, w['absent'] is not None, int(backwards),
                  w['speed'], w['reach']], np.int32).tobytes()
    b += np.array([w['dl']] + list(par6(w)), np.float64).tobytes()
    for k in I32_KEYS + OPT_KEYS:
        if w[k] is not None:
            b += w[k].tobytes()
    for k in F64_KEYS:
        b += w[k].tobytes()
    return b + (w['xref'].tobytes() if W else b'')


OUT_KEYS = ('leader', 'cut_len', 'gap', 'cap')


def out_bytes(w, got):
    """what the stand-alone program writes for a case whose words after both stages are w"""
    b = b''.join(w[k].tobytes() for k in OUT_KEYS) if len(w['traj_idx']) else b''
    if len(w['traj_idx']) and w.get('xref') is not None:
        b += w['xref'].tobytes()
    return b + np.array([got], np.int32).tobytes()


# ---------------------------------------------------------------- hand-made words
HAND = dict(dl=0.5, standstill=2.0, time_gap=1.0, brake=2.0, v_min=0.5, lateral=1.0, heading=0.5)
ROW2 = np.array([6.9, 6.9, 3.0, 0.5, 0.0, 0.0])      # a speed profile over a window of six points: cruise, a lower entry, a stop


def hand_made(speed, reach=20):
    """Hand-made words.  Path A = points 0..59 of the table, the x axis from 0 in steps of dl = 0.5 with heading 0: a car at x metres projects
    onto k = 2 x.  Path B = points 60..75: sixteen points of the same line.  standstill 2 m (4 points), time gap 1 s, brake 2, v_min 0.5,
    lateral 1 m, heading 0.5 rad, reach 20 points.  Every agent has a window of its own in the pool: its own row first, then its others.
    An agent is (route, traj_idx, v, cut_len, done, others); an other is (x, y, v, yaw) or the same with a fifth entry 1 = absent.
    With v = 2 the cut mode stops ceil((2 + 2) / 0.5) = 8 points behind the leader, the speed mode ceil(2 / 0.5) = 4.
    The cap is -2 + sqrt(4 + v_l^2 + 4 max(gap - 2, 0)), at least 0.5.
    Returns (words, want): want[q] = None or (slot of the leader among the agent's others, gap, cut_len in cut mode, in speed mode, cap)."""
    A, B = (0, 60), (60, 16)
    far = [(14.0 + 0.5 * j, 0.0, 1.0, 0.0) for j in range(15)]          # fifteen cars from k = 28 on: one in the scan (28, 29, 30), most beyond it
    rows = [
        (A, 10, 2.0, 60, 0, [], None),                                                  # 0  no others
        (A, 10, 2.0, 60, 0, [(10.0, 0.2, 3.0, 0.1)], (0, 5.0, 12, 16, 3.0)),            # 1  one other at k = 20: sqrt(4 + 9 + 12) - 2
        (A, 10, 2.0, 60, 0, [(14.0, 0.0, 9.0, 0.0), (2.0, 0.0, 9.0, 0.0), (5.0, 0.8, 9.0, 0.0), (12.0, 0.3, 5.0, -0.2), (13.0, 0.0, 9.0, 0.0),
                             (12.5, 3.0, 9.0, 0.0), (16.5, 0.0, 9.0, 0.0)], (3, 7.0, 16, 20, 5.0)),   # 2  seven others, the nearest ahead is k = 24
        (A, 10, 2.0, 60, 0, far + [(13.0, -0.1, 6.0, 0.0)], (15, 8.0, 18, 22, 6.0)),    # 3  sixteen others, the leader in the last slot: k = 26
        (A, 10, 2.0, 60, 0, [(2.0, 0.0, 1.0, 0.0)], None),                              # 4  a car behind: it projects onto k = traj_idx
        (A, 10, 2.0, 60, 0, [(5.0, 0.8, 1.0, 0.0)], None),                              # 5  a car beside
        (A, 10, 2.0, 60, 0, [(10.0, 0.0, 1.0, 1.5707963267948966)], None),              # 6  a car crossing: heading refused
        (A, 10, 2.0, 60, 0, [(10.0, 0.0, 1.0, 3.1)], None),                             # 7  an oncoming car
        (A, 10, 2.0, 60, 0, [(10.0, 1.0, 0.0, 0.0)], (0, 5.0, 12, 16, 2.0)),            # 8  exactly on the lateral bound: sqrt(4 + 0 + 12) - 2
        (A, 10, 2.0, 60, 0, [(10.0, 1.0000000000000002, 0.0, 0.0)], None),              # 9  one ulp beyond it
        (A, 10, 2.0, 60, 0, [(10.0, 0.1, 3.0, 0.0), (10.0, -0.1, 0.0, 0.0)], (0, 5.0, 12, 16, 3.0)),   # 10 two cars at the same k*: the lower row
        (A, 10, 2.0, 60, 0, [(17.0, 0.0, 1.0, 0.0)], None),                             # 11 a leader beyond reach: k = 34 > 30, 2 m from the last point
        (B, 5, 2.0, 16, 0, [(5.5, 0.0, 1.0, 0.0)], (0, 3.0, 6, 7, 1.0)),                # 12 a path shorter than reach: k = 11; sqrt(4 + 1 + 4) - 2
        (B, 15, 2.0, 16, 0, [(7.5, 0.0, 1.0, 0.0)], None),                              # 13 traj_idx on the last point
        (A, 10, 2.0, 60, 0, [(10.0, 0.0, 1.0, 0.0, 1), (12.0, 0.0, 1.0, 0.0)], (1, 7.0, 16, 20, 3.0)),  # 14 an absent row at k = 20: sqrt(4 + 1 + 20) - 2
        (A, 10, 2.0, 60, 1, [(10.0, 0.0, 1.0, 0.0)], None),                             # 15 a done agent
        (A, 10, 2.0, 60, 0, [(6.5, 0.0, 0.0, 0.0)], (0, 1.5, 11, 11, 0.5)),             # 16 s clamped at traj_idx + 1; no room: the cap is v_min
        (A, 10, 2.0, 14, 0, [(12.0, 0.0, 1.0, 0.0)], (0, 7.0, 14, 14, 3.0)),            # 17 an existing shorter cut is kept
        (A, 10, 2.0, 60, 0, [(10.0, 0.0, -1.0, 0.0)], (0, 5.0, 12, 16, 2.0)),           # 18 a leader rolling back: v_l = 0
        (A, 10, -1.0, 60, 0, [(10.0, 0.0, 3.0, 0.0)], (0, 5.0, 16, 16, 3.0)),           # 19 the ego rolling back: v = 0, four points in both modes
        (A, 10, 2.0, 60, 0, [(10.0, 0.0, 3.0, 6.383185307179586)], (0, 5.0, 12, 16, 3.0)),   # 20 a heading of 2 pi + 0.1 is wrapped
        (A, 10, 2.0, 60, 0, [(10.0, 0.0, 3.0, float('nan'))], None),                    # 21 a heading that is no number
    ]
    table = np.zeros((76, 3)); table[:60, 0] = 0.5 * np.arange(60); table[60:, 0] = 0.5 * np.arange(16)
    obs6, off, cnt, skip, absent = [], [], [], [], []
    for route, ti, v, cut, done, others, _ in rows:
        off.append(len(obs6)); cnt.append(1 + len(others)); skip.append(len(obs6))
        obs6.append((table[route[0] + ti, 0], 0.0, v, 0.0, 0.0, 0.0)); absent.append(0)
        for o in others:
            obs6.append(tuple(o[:4]) + (0.0, 0.0)); absent.append(int(len(o) > 4))
    P = len(rows)
    state = np.array([[table[r[0][0] + r[1], 0], 0.0, r[2], 0.0] for r in rows])
    rng = np.random.default_rng(11)
    xref = rng.uniform(-50.0, 50.0, (P, 4, 6))
    xref[:, 2] = ROW2
    w = words(state=state, path=table, path_off=[r[0][0] for r in rows], path_len=[r[0][1] for r in rows], traj_idx=[r[1] for r in rows],
              cut_len=[r[3] for r in rows], done=[r[4] for r in rows], obs6=np.array(obs6), obs_off=off, obs_cnt=cnt, obs_skip=skip, absent=absent,
              xref=xref, speed=int(speed), reach=reach, **HAND)
    return w, [r[6] for r in rows]


def random_words(seed, P=None, speed=None, W=None):
    """a seeded scene: P agents (1..40 unless given) on curved paths of 20..120 points, each with a window of 0..16 others around its path
    -- ahead, behind, beside, oncoming, far, some absent, some rows shared with its neighbour's window --, some agents done, some windows
    out of the pool, W = 1..33 unless given"""
    rng = np.random.default_rng(seed)
    P = int(rng.integers(1, 41)) if P is None else int(P)
    W = int(rng.integers(1, 34)) if W is None else int(W)
    dl = float(rng.choice([0.083, 0.5, 1.0]))
    lens = rng.integers(20, 121, P)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    table = np.zeros((int(lens.sum()), 3))
    for q in range(P):
        yaw = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.uniform(-0.02, 0.02, lens[q]))
        table[offs[q]:offs[q] + lens[q], 2] = yaw
        table[offs[q]:offs[q] + lens[q], 0] = rng.uniform(-50, 50) + np.cumsum(np.cos(yaw) * dl)
        table[offs[q]:offs[q] + lens[q], 1] = rng.uniform(-50, 50) + np.cumsum(np.sin(yaw) * dl)
    ti = np.array([rng.integers(0, lens[q]) for q in range(P)])
    obs6, off, cnt, skip, absent = [], [], [], [], []
    for q in range(P):
        n = int(rng.integers(0, MAX_OBS + 1)) if rng.random() < 0.9 else int(rng.integers(MAX_OBS, MAX_OBS + 4))
        own_at = int(rng.integers(0, n + 1))
        off.append(len(obs6)); cnt.append(n + 1)
        for j in range(n + 1):
            if j == own_at:
                skip.append(len(obs6))
                obs6.append(np.concatenate([table[offs[q] + ti[q], :2], [rng.uniform(-1, 8), table[offs[q] + ti[q], 2], 0, 0]])); absent.append(0)
                continue
            k = int(np.clip(ti[q] + rng.integers(-10, 60), 0, lens[q] - 1))
            pt = table[offs[q] + k]
            side = rng.choice([0.0, 0.0, 0.3, 1.4, 1.6, 5.0]) * rng.choice([-1, 1])
            turn = rng.choice([0.0, 0.0, 0.3, 0.79, 0.81, np.pi, 2 * np.pi, -2 * np.pi + 0.1, 1.5])
            obs6.append([pt[0] - np.sin(pt[2]) * side, pt[1] + np.cos(pt[2]) * side, rng.uniform(-1, 8), pt[2] + turn, 0, 0])
            absent.append(int(rng.random() < 0.1))
    off, cnt = np.array(off), np.array(cnt)
    bad = rng.random(P) < 0.05
    off = np.where(bad, rng.integers(-3, len(obs6) + 3, P), off)          # windows that leave the pool
    cut = np.where(rng.random(P) < 0.3, ti + rng.integers(1, 8, P), lens)
    state = np.array([[table[offs[q] + ti[q], 0], table[offs[q] + ti[q], 1], rng.uniform(-1, 8), table[offs[q] + ti[q], 2]] for q in range(P)])
    xref = rng.uniform(0.0, 8.0, (P, 4, W)) * (rng.random((P, 4, W)) < 0.8)
    return words(state=state, path=table, path_off=offs, path_len=lens, traj_idx=ti, cut_len=cut,
                 done=(rng.random(P) < 0.15).astype(np.int32) if seed % 3 else None, obs6=np.array(obs6).reshape(-1, 6), obs_off=off, obs_cnt=cnt,
                 obs_skip=skip if seed % 5 else None, absent=absent if seed % 4 else None, xref=xref,
                 speed=int(seed & 1) if speed is None else int(speed), reach=int(rng.choice([1, 7, 16, 17, 40, 200])), dl=dl,
                 standstill=float(rng.uniform(0.5, 6.0)), time_gap=float(rng.uniform(0.0, 2.0)), brake=float(rng.uniform(1.0, 5.0)),
                 v_min=float(rng.uniform(0.1, 1.0)), lateral=float(rng.choice([0.3, 1.5, 1.6])), heading=float(rng.choice([0.3, 0.8, 3.2])))


# ---------------------------------------------------------------- the oracle step
def follow_agent_step(p, full, dl, st, rows, traj_idx, prev, target, u, centers, radius, margin, speed, follow, decide=None, advise=None,
                      v_ref=S.V_REF):
    """One agent's step under the rule, beside signals and advice where decide / advise are given: orc.agent_step (speedref_helpers.agent_step
    in speed mode); then decide(traj_idx, v) -> (held, line) as signal_helpers.signal_agent_step has it; then follow(traj_idx, v) -> None or
    (leader, gap, s, cap) on the traj_idx the step returned; then advise(traj_idx, cut) -> the advised speed on the cut both left.  Where the
    cut moved or a cap applies, only the window, rollout and QP again on full[:cut] (speed mode: the whole path with the speed profile zeroed
    from cut on and capped at the advised speed and the follower's cap), with the pieces agent_step itself calls.  Returns agent_step's
    dict with `cut` (speed mode: the stop index, 999 = none), `held`, `leader`, `gap`, `cap`, `advised` and the sol / target_ind that hold."""
    full = np.ascontiguousarray(full, np.float64)
    if speed:
        r = S.agent_step(p, full, dl, st, rows, traj_idx, prev, target, u, centers, radius, margin, v_ref=v_ref)
        cut0 = r['stop']
    else:
        r = orc.agent_step(p, full, dl, st, rows, traj_idx, prev, target, u, centers, radius, margin)
        cut0 = r['cut']
    ti, cut = int(r['traj_idx']), int(cut0)
    held, line = (0, -1) if decide is None else decide(ti, st[2])
    if held and line < cut:
        cut = int(line)
    f = follow(ti, st[2])
    leader, gap, cap = (-1, -1.0, 0.0) if f is None else (f[0], f[1], f[3])
    if f is not None and f[2] < cut:
        cut = int(f[2])
    advised = 0.0 if advise is None or not speed else float(advise(ti, cut))
    r = dict(r, held=int(held), line=int(line), leader=int(leader), gap=float(gap), cap=float(cap), advised=advised, xref_free=r['xref'])
    if cut != cut0 or (speed and (cap > 0.0 or advised > 0.0)):
        uw = np.zeros((2, p.T)) if u is None else np.asarray(u, float)
        if speed:
            cv = S.speed_profile(len(full), cut, v_ref=v_ref)
            if advised > 0.0:
                cv = np.minimum(cv, advised)
            if cap > 0.0:
                cv = np.minimum(cv, cap)
            xref, tgt, re = orc.calc_ref_trajectory(p, st, full[:, 0], full[:, 1], full[:, 2], dl, target, cv=cv)
        else:
            tmp = full[:cut]
            xref, tgt, re = orc.calc_ref_trajectory(p, st, tmp[:, 0], tmp[:, 1], tmp[:, 2], dl, target)
        assert tgt >= 0
        xbar = orc.predict_motion(p, list(st), uw[0], uw[1])
        r.update(target_ind=tgt, xref=xref, xbar=xbar, re=re, sol=orc.qp_solve(p, list(st), xref, xbar, re, uw))
    r['cut'] = int(cut)
    return r


# ---------------------------------------------------------------- the oracle loop
class FollowOracleLoop(G.SignalOracleLoop):
    """SignalOracleLoop with the following rule.  follow: dict(standstill, time_gap, brake, v_min, lateral, heading, reach) or None (= the
    run without it, with the same records); plan None: no signals.  Records per step leader, gap and cap, the true clearance between the
    present, driving agents and the scripted rows at the start of every step (worst_clearance) and the steps with a contact (clearance < 0)."""

    def __init__(self, paths, dl, start, stop=None, group=None, plan=None, follow=FOLLOW, **kw):
        free = plan is None
        if free:
            plan = dict(cycle=1, amber=0, green=np.array([[0, 1]]))
            stop = [np.full(len(p), -1, np.int32) for p in paths]
            group = [np.zeros(len(p), np.int32) for p in paths]
        super().__init__(paths, dl, start, stop, group, plan, **kw)
        self.follow, self.signalled = follow, not free
        self.contacts, self.followed_steps = [], 0

    def _measure(self, pool):
        live = [a for a in range(self.A) if not self.done[a] and not self.absent[a]]
        rows = live + list(range(self.A, len(pool)))
        for a in live:
            others = [r for r in rows if r != a]
            if others:
                c = SH.clearance(pool, a, others, self.centers, self.radius)
                self.worst_clearance = min(self.worst_clearance, c)
                if c < 0 and self.steps not in self.contacts:
                    self.contacts.append(self.steps)

    def _follow(self, a, pool, present, ti, v):
        if self.follow is None:
            return None
        best = leader_of(np.asarray(self.paths[a], np.float64), ti, pool, present[:MAX_OBS], self.follow, self.follow['reach'])
        if best is None:
            return None
        gap, s, cap = stop_and_cap(ti, best[1], best[2], v, self.dl, self.speed, self.follow)
        return best[0], gap, s, cap

    def step(self):
        A = self.A
        pool = self.pool()
        self._measure(pool)
        gone = list(self.absent) + [False] * (len(pool) - A)
        out = [None] * A
        new_state, new_applied = self.state.copy(), self.applied.copy()
        arrived = []
        for a in range(A):
            if self.done[a]:
                self.held[a] = 0
                continue
            present = [r for r in range(len(pool)) if r != a and not gone[r]]
            full = self.paths[a]
            st = self.state[a]
            r = follow_agent_step(self.p, full, self.dl, st, pool[present], self.traj_idx[a], self.prev[a], self.target[a], self.u[a], self.centers,
                                  self.radius, self.margin, self.speed, lambda ti, v, a=a, present=present: self._follow(a, pool, present, ti, v),
                                  decide=(lambda ti, v, a=a: self._decide(a, ti, v)) if self.signalled else None)
            held, cut, sol, target = r['held'], r['cut'], r['sol'], r['target_ind']
            self.held[a] = held
            self.followed_steps += r['leader'] >= 0
            length = len(full) if self.speed else cut
            assert sol.status == 0, (self.steps, a, sol.status)
            post = np.asarray(orc.plant_step(self.p, st, sol.u[0, 0], sol.u[1, 0]), dtype=np.float64)
            self.traj_idx[a], self.target[a], self.prev[a], self.u[a] = int(r['traj_idx']), int(target), int(length), sol.u.copy()
            new_state[a] = post
            new_applied[a] = (sol.u[1, 0], sol.u[0, 0])
            out[a] = dict(pool=pool, present=present, hit=-1 if r['hit'] is None else int(r['hit'][2]), cut=int(cut), goal_len=int(length),
                          target=int(target), traj_idx=int(r['traj_idx']), x_sol=sol.x.copy(), u_sol=sol.u.copy(), post=post.copy(),
                          ctrl=new_applied[a].copy(), status=int(sol.status), held=int(held), leader=r['leader'], gap=r['gap'], cap=r['cap'])
            if SH.is_goal(post, full[-1], target, length):
                arrived.append(a)
        self.tick = [(t % self.plan['cycle'] + 1) % self.plan['cycle'] for t in self.tick]
        self.state, self.applied = new_state, new_applied
        self.steps += 1
        for a in arrived:
            self.done[a], self.arrival[a] = True, self.steps
            self.applied[a] = 0.0
            if self.depart:
                self.absent[a] = True
        return out


# ---------------------------------------------------------------- the scenes
QUEUE_LINE = 500        # the stop line of the queue scene: 41.5 m along the route


def queue_scene(n=5, spacing=100):
    """n cars on the straight stock route from the south, `spacing` points (8.3 m) apart, the first one `spacing` points before a stop line
    at point QUEUE_LINE: (paths, dl, start, stop, group)"""
    paths, dl, _, _, _ = G.straight_scene()
    L = len(paths[0])
    stop = np.where(np.arange(L) <= QUEUE_LINE, QUEUE_LINE, -1).astype(np.int32)
    start = [QUEUE_LINE - spacing * (a + 1) for a in range(n)]
    return [paths[0]] * n, dl, start, [stop] * n, [np.zeros(L, np.int32)] * n


def queue_loop(speed, follow=FOLLOW, n=5):
    """four cars on one straight route behind a leader that a red light holds at its line for the whole run (a plan whose only group is never
    green), in cut mode or in speed mode"""
    paths, dl, start, stop, group = queue_scene(n)
    plan = dict(cycle=100, amber=0, green=np.array([[0, 0]]))
    return FollowOracleLoop(paths, dl, start, stop, group, plan, follow=follow, T=13, depart=True, speed=speed)


def merge_loop(follow=FOLLOW, speed=False, back=(26.0, 34.0)):
    """two routes that share an exit arm (scene_helpers.shared_exit_setup), the cars `back` metres before their last points"""
    paths, dl, start = SH.shared_exit_setup(*back)
    return FollowOracleLoop(paths, dl, start, follow=follow, T=13, depart=True, speed=speed)
