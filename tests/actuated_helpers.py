"""Vehicle-actuated signals (mpcx_actuation: a controller per junction decides the lights from who is waiting; the hold at the line is the
signal rule's) for the tests: a numpy restatement of the rule, the host build of csrc/mpcx_actuated_core.h
(tests/actuated_ref/actuated_ref.cpp) behind numpy arrays, the hand-made junctions of tests/test_actuated_cpu.py and the closed loop of
several egos on the CPU oracle under the rule (ActuatedOracleLoop, a subclass of signal_helpers.SignalOracleLoop in which the junction's
state machine replaces the clock)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import signal_helpers as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'actuated_ref', 'actuated_ref.cpp')
INC = G.INC
GREEN, AMBER, RED = G.GREEN, G.AMBER, G.RED
ST_GREEN, ST_AMBER, ST_ALL_RED = 0, 1, 2

# the controller tests/test_actuated_cpu.py runs on the straight scene: min_green 10, max_green 40, gap 5, amber 8, all_red 12 (the amber
# and all-red of signal_helpers.PLAN)
CONTROLLER = dict(min_green=10, max_green=40, gap=5, amber=8, all_red=12)


# ---------------------------------------------------------------- the rule restated
def lights_word(mask, stage, n_groups):
    """step 2: 2 bits per group"""
    w = 0
    for g in range(n_groups):
        on = stage != ST_ALL_RED and (mask >> g) & 1
        w |= ((GREEN if stage == ST_GREEN else AMBER) if on else RED) << (2 * g)
    return w


def read_state(word, n_phases):
    """step 1: a defective word counts as (0, GREEN, 0, 0)"""
    p, stage, timer, idle = (int(v) for v in word)
    if not 0 <= p < n_phases or stage not in (0, 1, 2) or timer < 0 or idle < 0:
        return 0, ST_GREEN, 0, 0
    return p, stage, timer, idle


def advance(masks, times, ctrl, st, calls):
    """step 4: masks (n_phases,), times (n_phases, 3) = (min_green, max_green, gap), ctrl = (amber, all_red, detect); st as read"""
    p, stage, timer, idle = st
    n = len(masks)
    D = [(calls & int(m)) != 0 for m in masks]
    ring = [(p + d) % n for d in range(1, n)]
    called = [k for k in ring if D[k]]
    nxt = called[0] if called else (p + 1) % n
    amber, all_red = int(ctrl[0]), int(ctrl[1])
    if stage == ST_GREEN:
        mn, mx, gap = (int(v) for v in times[p])
        timer = min(timer + 1, mx)
        idle = 0 if D[p] else min(idle + 1, gap)
        if not (bool(called) and timer >= mn and (idle >= gap or timer >= mx)):
            return p, ST_GREEN, timer, idle
        stage = ST_AMBER
    else:
        timer += 1
        if timer < (amber if stage == ST_AMBER else all_red):
            return p, stage, timer, idle
        stage += 1
    # entered `stage` with timer 0: a stage of length 0 is passed through in the same step
    if stage == ST_AMBER and amber == 0:
        stage = ST_ALL_RED
    if stage == ST_ALL_RED and all_red == 0:
        stage = ST_ALL_RED + 1
    if stage > ST_ALL_RED:
        return nxt, ST_GREEN, 0, 0
    return p, stage, 0, 0


def call_bit(w, q, detect):
    """step 3 for agent q: its call bit or 0"""
    if w.get('done') is not None and w['done'][q]:
        return 0
    ti = int(w['traj_idx'][q])
    i = int(w['path_off'][q]) + ti
    if not 0 <= i < len(w['path_stop']):
        return 0
    s, g = int(w['path_stop'][i]), int(w['path_group'][i])
    if not 0 <= s < int(w['path_len'][q]) or ti >= s or not 0 <= g < int(w['n_groups']):
        return 0
    return 1 << g if s - ti <= detect else 0


def hold(w, q, lit, lights):
    """step 5 = steps 2 - 5 of the signal rule for agent q with the light of its group from the word `lights`; in place, returns held"""
    if w.get('done') is not None and w['done'][q]:
        w['held'][q] = 0
        return 0
    ti = int(w['traj_idx'][q])
    i = int(w['path_off'][q]) + ti
    held = 0
    if lit and 0 <= i < len(w['path_stop']):
        s, g = int(w['path_stop'][i]), int(w['path_group'][i])
        if 0 <= s < int(w['path_len'][q]) and ti < s and 0 <= g < int(w['n_groups']):
            lt = (lights >> (2 * g)) & 3
            if lt == RED:
                held = 1
            elif lt == AMBER:
                v = np.float64(w['state'][q, 2])
                if w['held'][q] != 0 or np.float64(s - ti) * np.float64(w['dl']) >= v * v / (np.float64(2.0) * np.float64(w['brake'])):
                    held = 2
            if held and s < w['cut_len'][q]:
                w['cut_len'][q] = s
    w['held'][q] = held
    return held


def rule_numpy(w, backwards=False):
    """the rule restated on a dict of numpy arrays (words()), in place on jstate, lights, calls, held and cut_len; returns the agents held"""
    n_per, J = int(w['n_per']), len(w['ctrl_of'])
    n_ctrl, n_phases = w['phase_groups'].shape
    got = 0
    for j in (range(J - 1, -1, -1) if backwards else range(J)):
        k = int(w['ctrl_of'][j])
        agents = range(j * n_per, (j + 1) * n_per)
        lights = calls = 0
        lit = 0 <= k < n_ctrl
        if lit:
            st = read_state(w['jstate'][j], n_phases)
            lights = lights_word(int(w['phase_groups'][k, st[0]]), st[1], int(w['n_groups']))
            for q in agents:
                calls |= call_bit(w, q, int(w['ctrl_time'][k, 2]))
            w['jstate'][j] = advance(w['phase_groups'][k], w['phase_time'][k], w['ctrl_time'][k], st, calls)
        w['lights'][j], w['calls'][j] = lights, calls
        for q in agents:
            got += hold(w, q, lit, lights) != 0
    return got


# ---------------------------------------------------------------- the host build
def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libactuated_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.actuated_ref_step.restype = C.c_int
    lib.actuated_ref_step.argtypes = ([C.c_int, C.c_double] + [C.c_void_p] * 9 + [C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 7 +
                                      [C.c_int] * 5)
    lib.actuated_ref_layout.restype = None
    return lib


I32_KEYS = ('path_off', 'path_len', 'traj_idx', 'cut_len', 'path_stop', 'path_group', 'held', 'phase_groups', 'phase_time', 'ctrl_time', 'ctrl_of',
            'jstate', 'lights', 'calls')
OUT_KEYS = ('jstate', 'lights', 'calls', 'held', 'cut_len')


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes: per agent state (P, 4), path_off, path_len, traj_idx,
    cut_len, done (or None), held; per path point path_stop, path_group; phase_groups (n_ctrl, n_phases), phase_time (n_ctrl, n_phases, 3),
    ctrl_time (n_ctrl, 3); per junction ctrl_of, jstate (J, 4), lights, calls; scalars dl, brake, n_groups, n_per"""
    w = dict(kw)
    for k in I32_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    w['state'] = np.ascontiguousarray(w['state'], dtype=np.float64)
    w['done'] = None if w.get('done') is None else np.ascontiguousarray(w['done'], dtype=np.int32)
    assert w['jstate'].shape == (len(w['ctrl_of']), 4) and len(w['held']) == int(w['n_per']) * len(w['ctrl_of'])
    return w


def host_rule(lib, w, backwards=False):
    """the rule through the host build, in place on OUT_KEYS of w (a dict from words()); returns the number held"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    n_ctrl, n_phases = w['phase_groups'].shape
    return lib.actuated_ref_step(len(w['held']), float(w['dl']), p('state'), p('path_off'), p('path_len'), p('traj_idx'), p('cut_len'), p('done'),
                                 p('path_stop'), p('path_group'), p('held'), float(w['brake']), len(w['path_stop']), int(w['n_groups']),
                                 p('phase_groups'), p('phase_time'), p('ctrl_time'), p('ctrl_of'), p('jstate'), p('lights'), p('calls'),
                                 int(w['n_per']), len(w['ctrl_of']), n_phases, n_ctrl, int(backwards))


def copy_words(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def blob(w, backwards):
    """a case of the stand-alone program's input file"""
    n_ctrl, n_phases = w['phase_groups'].shape
    b = np.array([len(w['held']), len(w['path_stop']), w['n_groups'], w['n_per'], len(w['ctrl_of']), n_phases, n_ctrl, int(w['done'] is not None),
                  int(backwards)], np.int32).tobytes()
    b += np.array([w['dl'], w['brake']], np.float64).tobytes() + w['state'].tobytes()
    for k in ('path_off', 'path_len', 'traj_idx', 'cut_len'):
        b += w[k].tobytes()
    if w['done'] is not None:
        b += w['done'].tobytes()
    for k in ('path_stop', 'path_group', 'held', 'phase_groups', 'phase_time', 'ctrl_time', 'ctrl_of', 'jstate', 'lights', 'calls'):
        b += w[k].tobytes()
    return b


def out_bytes(w, got):
    """what the stand-alone program writes for a case"""
    return b''.join(w[k].tobytes() for k in OUT_KEYS) + np.array([got], np.int32).tobytes()


# ---------------------------------------------------------------- the hand-made junctions
# Three routes in a table of 80 points: A = points 0..29 with its line at local index 20 (group 0), B = points 30..49 with its line at local
# index 10 (group 1), C = points 50..79 with its line at local index 15 (group 2); nothing behind a line.  dl = 0.5, brake = 2: a car at v
# stops within v v / 4 metres.  Four controllers over three phases, one group each (masks 1, 2, 4), every phase (min_green 3, max_green 6,
# gap 2), detect 8 points; they differ in (amber, all_red): controller 0 (2, 1), 1 (0, 1), 2 (2, 0), 3 (0, 0).
# Light words (2 bits per group, group 0 lowest; GREEN 0, AMBER 1, RED 2): all red 42; phase 0 green 40, amber 41; phase 1 green 34, amber
# 38; phase 2 green 10, amber 26.
A_, B_, C_ = (0, 30), (30, 20), (50, 30)
a0 = (A_, 15, 3.0, 30, 0, 0)          # (route, traj_idx, v, cut, held, done): 5 points before line 20 -- calls group 0
b1 = (B_, 5, 1.0, 20, 0, 0)           # 5 points before line 10 -- calls group 1
c2 = (C_, 10, 1.0, 30, 0, 0)          # 5 points before line 15 -- calls group 2
PAD = (B_, 12, 1.0, 20, 0, 0)         # behind its line: no line ahead, never calls, never held (fills a junction up to n_per)
G_, Y_, R_ = ST_GREEN, ST_AMBER, ST_ALL_RED

CASES = [
    # (what, controller, jstate as read, agents) -> want (jstate, lights, calls, [(held, cut) per agent])
    # ---- transitions
    ('minimum green holds although the gap has run out', 0, (0, G_, 0, 2), [b1], ((0, G_, 1, 2), 40, 2, [(1, 10)])),
    ('gap-out: timer 3 >= min, idle 2 >= gap, group 1 waits', 0, (0, G_, 2, 1), [b1], ((0, Y_, 0, 0), 40, 2, [(1, 10)])),
    ('own demand resets idle: no gap-out, not yet max', 0, (0, G_, 4, 1), [a0, b1], ((0, G_, 5, 0), 40, 3, [(0, 30), (1, 10)])),
    ('max-out under continuous own demand', 0, (0, G_, 5, 0), [a0, b1], ((0, Y_, 0, 0), 40, 3, [(0, 30), (1, 10)])),
    ('rest in green, own call only: the timer stays at max', 0, (0, G_, 6, 2), [a0], ((0, G_, 6, 0), 40, 1, [(0, 30)])),
    ('rest in green, nobody calls', 0, (0, G_, 6, 2), [], ((0, G_, 6, 2), 40, 0, [])),
    ('rest in green past max and gap: only own phase called', 1, (1, G_, 6, 0), [b1], ((1, G_, 6, 0), 34, 2, [(0, 20)])),
    ('phase 1 without a call is skipped: 0 -> 2', 0, (0, R_, 0, 0), [c2], ((2, G_, 0, 0), 42, 4, [(1, 15)])),
    ('ring order wraps: from 2 the first called is 1 (0 is not)', 0, (2, R_, 0, 0), [b1], ((1, G_, 0, 0), 42, 2, [(1, 10)])),
    ('ring order: from 1, 2 comes before 0', 0, (1, R_, 0, 0), [a0, c2], ((2, G_, 0, 0), 42, 5, [(1, 20), (1, 15)])),
    ('own call alone does not pick the own phase: fall-back to p + 1', 0, (1, R_, 0, 0), [b1], ((2, G_, 0, 0), 42, 2, [(1, 10)])),
    ('fall-back to p + 1 when no phase calls', 0, (0, R_, 0, 0), [], ((1, G_, 0, 0), 42, 0, [])),
    ('fall-back wraps: 2 -> 0', 0, (2, R_, 0, 0), [], ((0, G_, 0, 0), 42, 0, [])),
    ('amber counts', 0, (1, Y_, 0, 0), [a0], ((1, Y_, 1, 0), 38, 1, [(1, 20)])),
    ('amber ends at 2: all red', 0, (1, Y_, 1, 0), [a0], ((1, R_, 0, 0), 38, 1, [(1, 20)])),
    ('amber = 0: gap-out goes straight to all red', 1, (0, G_, 2, 1), [b1], ((0, R_, 0, 0), 40, 2, [(1, 10)])),
    ('all_red = 0: the end of amber is the next green', 2, (0, Y_, 1, 0), [b1], ((1, G_, 0, 0), 41, 2, [(1, 10)])),
    ('all_red = 0: gap-out enters amber as usual', 2, (0, G_, 2, 1), [b1], ((0, Y_, 0, 0), 40, 2, [(1, 10)])),
    ('both 0: gap-out is the next green', 3, (0, G_, 2, 1), [c2], ((2, G_, 0, 0), 40, 4, [(1, 15)])),
    ('both 0: an all-red word read leaves at once', 3, (0, R_, 0, 0), [], ((1, G_, 0, 0), 42, 0, [])),
    ('defective word: phase 5 of 3 counts as (0, GREEN, 0, 0)', 0, (5, G_, 0, 0), [b1], ((0, G_, 1, 1), 40, 2, [(1, 10)])),
    ('defective word: stage 3', 0, (1, 3, 2, 0), [b1], ((0, G_, 1, 1), 40, 2, [(1, 10)])),
    ('defective word: negative timer', 0, (1, Y_, -1, 0), [a0], ((0, G_, 1, 0), 40, 1, [(0, 30)])),
    ('defective word: negative idle', 0, (2, G_, 4, -4), [], ((0, G_, 1, 1), 40, 0, [])),
    # ---- detector
    ('ctrl_of = 4 of 4: no controller, jstate left alone, a hold is dropped', 4, (1, Y_, 1, 0), [(B_, 5, 1.0, 20, 1, 0)], ((1, Y_, 1, 0), 0, 0, [(0, 20)])),
    ('ctrl_of = -1', -1, (7, 7, 7, 7), [a0], ((7, 7, 7, 7), 0, 0, [(0, 30)])),
    ('s - traj_idx = 8 = detect calls', 0, (0, G_, 0, 0), [(A_, 12, 3.0, 30, 0, 0)], ((0, G_, 1, 0), 40, 1, [(0, 30)])),
    ('s - traj_idx = 9 = detect + 1 does not (and is still held at red)', 0, (1, G_, 0, 0), [(A_, 11, 3.0, 30, 0, 0)], ((1, G_, 1, 1), 34, 0, [(1, 20)])),
    ('a done agent does not call: no gap-out; its hold is cleared, its cut kept', 0, (0, G_, 2, 1), [(B_, 5, 1.0, 20, 1, 1)], ((0, G_, 3, 2), 40, 0, [(0, 20)])),
    ('on and past the line: no call, free at red', 0, (1, G_, 0, 0), [(A_, 20, 3.0, 30, 1, 0), (A_, 22, 3.0, 30, 0, 0)], ((1, G_, 1, 1), 34, 0, [(0, 30), (0, 30)])),
    ('defective points: group 7 of 3; s = 25 >= path_len = 20', 0, (0, G_, 0, 0), [(B_, 15, 1.0, 20, 0, 0), (B_, 16, 1.0, 20, 0, 0)], ((0, G_, 1, 1), 40, 0, [(0, 20), (0, 20)])),
    ('defective points: i = 83 outside [0, 80); i = -4', 0, (0, G_, 0, 0), [((78, 30), 5, 3.0, 30, 0, 0), ((-9, 30), 5, 3.0, 30, 0, 0)], ((0, G_, 1, 1), 40, 0, [(0, 30), (0, 30)])),
    # ---- hold under an actuated light
    ('amber: can stop (5 >= 16 / 4), cannot stop (5 < 25 / 4), cannot but held before: sticky', 0, (0, Y_, 0, 0),
     [(A_, 10, 4.0, 30, 0, 0), (A_, 10, 5.0, 30, 0, 0), (A_, 10, 5.0, 30, 2, 0)], ((0, Y_, 1, 0), 41, 0, [(2, 20), (0, 30), (2, 20)])),
    ('red with a conflict cut shorter than the line: kept', 0, (1, G_, 0, 0), [(A_, 15, 3.0, 12, 0, 0)], ((1, G_, 1, 1), 34, 1, [(1, 12)])),
    ('all red holds every group; a previous hold at amber becomes one at red', 0, (1, R_, 0, 0), [(B_, 5, 1.0, 20, 2, 0)], ((2, G_, 0, 0), 42, 2, [(1, 10)])),
]


def _tables():
    stop = np.full(80, -1, np.int32); grp = np.zeros(80, np.int32)
    stop[0:21] = 20; stop[30:41] = 10; grp[30:41] = 1; stop[50:66] = 15; grp[50:66] = 2
    grp[45] = 7; stop[45] = 18            # a defective point: a group that does not exist
    stop[46] = 25                         # a defective point: a line beyond the route's end
    stop[22] = 20                         # a table that still names the line behind the point: past the line
    return stop, grp


def slots(n_agents, n_per):
    """where a case's agents sit in a junction of n_per: the last slot, the first, the middle -- at n_per = 70 the last is reached in the
    second round of the kernel's stride loop, at n_per = 3 the lane group has a padding lane"""
    return [n_per - 1, 0, n_per // 2][:n_agents]


def hand_made(n_per, repeat=1):
    """CASES as junctions of n_per agents (the cases with more agents than n_per are left out: at n_per = 1 a junction cannot hold a
    contest), `repeat` times over; returns (words, want) with want = (jstate (J, 4), lights (J,), calls (J,), {agent: (held, cut)})"""
    stop, grp = _tables()
    cases = [c for c in CASES if len(c[3]) <= n_per] * repeat
    J = len(cases)
    rows = [PAD] * (J * n_per)
    want_agent = {}
    for j, (_, _, _, agents, want) in enumerate(cases):
        for slot, ag, wa in zip(slots(len(agents), n_per), agents, want[3]):
            rows[j * n_per + slot] = ag
            want_agent[j * n_per + slot] = wa
    P = len(rows)
    state = np.zeros((P, 4)); state[:, 2] = [r[2] for r in rows]
    timing = np.tile(np.array([3, 6, 2]), (4, 3, 1))
    w = words(state=state, path_off=[r[0][0] for r in rows], path_len=[r[0][1] for r in rows], traj_idx=[r[1] for r in rows],
              cut_len=[r[3] for r in rows], held=[r[4] for r in rows], done=[r[5] for r in rows], path_stop=stop, path_group=grp,
              phase_groups=np.tile(np.array([1, 2, 4]), (4, 1)), phase_time=timing, ctrl_time=[[2, 1, 8], [0, 1, 8], [2, 0, 8], [0, 0, 8]],
              ctrl_of=[c[1] for c in cases], jstate=np.array([c[2] for c in cases]).reshape(J, 4), lights=np.full(J, -1), calls=np.full(J, -1),
              dl=0.5, brake=2.0, n_groups=3, n_per=n_per)
    want = (np.array([c[4][0] for c in cases], np.int32).reshape(J, 4), np.array([c[4][1] for c in cases], np.int32),
            np.array([c[4][2] for c in cases], np.int32), want_agent)
    return w, want


def check_against_want(w, want, rows):
    """the words after the rule against the hand-written expectations; rows: the agents' (route, traj_idx, v, cut, held, done) before"""
    js, li, ca, ag = want
    assert np.array_equal(w['jstate'], js), np.flatnonzero((w['jstate'] != js).any(axis=1))
    assert np.array_equal(w['lights'], li), np.flatnonzero(w['lights'] != li)
    assert np.array_equal(w['calls'], ca), np.flatnonzero(w['calls'] != ca)
    for q in range(len(w['held'])):
        held, cut = ag.get(q, (0, rows['cut_len'][q]))        # (a padding agent is never held and keeps its cut)
        assert (w['held'][q], w['cut_len'][q]) == (held, cut), (q, w['held'][q], w['cut_len'][q], held, cut)


# ---------------------------------------------------------------- the oracle loop
def controller_tables(ct):
    """a controller dict (batch.two_phase_controller) as (masks (n_phases,), times (n_phases, 3), ctrl (3,)) of Python ints"""
    n = len(ct['phases'])
    masks = [sum(1 << int(g) for g in set(ph)) for ph in ct['phases']]
    per = lambda v: [int(x) for x in (np.full(n, v) if np.ndim(v) == 0 else v)]
    times = list(zip(per(ct['min_green']), per(ct['max_green']), per(ct['gap'])))
    return masks, times, (int(ct['amber']), int(ct['all_red']), int(ct['detect']))


class ActuatedOracleLoop(G.SignalOracleLoop):
    """SignalOracleLoop with ONE junction's state machine in the place of the clock.  controller: a dict as batch.two_phase_controller
    builds it.  The lights of a step come from the junction state at its start; every driving agent's call is taken from the traj_idx its
    conflict search returned (the kernel's order: the stage runs behind the conflict search); the state advances at the end of the step.
    Records per step the light word (lights_hist), the calls (calls_hist) and the state the step started from (jstate_hist)."""

    def __init__(self, paths, dl, start, stop, group, controller, n_groups=4, **kw):
        self.masks, self.times, self.ctrl = controller_tables(controller)
        phase_of_group = [next((k for k, m in enumerate(self.masks) if (m >> g) & 1), -1) for g in range(n_groups)]
        # (the parent reads its plan for two things only: which agents share a phase -- equal `green` rows -- and the clock it advances)
        super().__init__(paths, dl, start, stop, group, dict(cycle=1, amber=0, green=[[k, 0] for k in phase_of_group]), **kw)
        self.n_groups = n_groups
        self.jstate = (0, ST_GREEN, 0, 0)
        self.lights, self.calls = 0, 0
        self.lights_hist, self.calls_hist, self.jstate_hist = [], [], []

    def _decide(self, a, ti, v):
        s, g = int(self.stop[a][ti]), int(self.group[a][ti])
        if s < 0 or ti >= s or s >= len(self.paths[a]) or not 0 <= g < self.n_groups:
            return 0, s
        if s - ti <= self.ctrl[2]:
            self.calls |= 1 << g
        lt = (self.lights >> (2 * g)) & 3
        if lt == RED:
            return 1, s
        if lt == AMBER and (self.held[a] != 0 or np.float64(s - ti) * np.float64(self.dl) >= np.float64(v) * np.float64(v) / (2.0 * self.brake)):
            return 2, s
        self.amber_free += lt == AMBER
        return 0, s

    def step(self):
        st = read_state(self.jstate, len(self.masks))
        self.lights, self.calls = lights_word(self.masks[st[0]], st[1], self.n_groups), 0
        out = super().step()
        self.jstate_hist.append(tuple(self.jstate)); self.lights_hist.append(self.lights); self.calls_hist.append(self.calls)
        self.jstate = advance(self.masks, self.times, self.ctrl, st, self.calls)
        return out


def straight_loop(controller, arms=(1, 2, 3, 4)):
    """the straight scene of signal_helpers (T = 13, v0 = 0, cut mode, departure on) under an actuated controller; arms: the approach arms
    that have a car"""
    paths, dl, start, stop, group = G.straight_scene()
    keep = [a - 1 for a in arms]
    pick = lambda t: [t[k] for k in keep]
    return ActuatedOracleLoop(pick(paths), dl, pick(start), pick(stop), pick(group), controller, T=13, depart=True)


def line_index():
    """the largest stop-line index of the straight scene: a detector at least this long sees a car from its start"""
    return max(int(s[0]) for s in G.straight_scene()[3])


def junctions(w, j0, j1):
    """the words of junctions [j0, j1) alone (the tables stay whole)"""
    n = int(w['n_per'])
    out = dict(w)
    for k in ('state', 'path_off', 'path_len', 'traj_idx', 'cut_len', 'held', 'done'):
        out[k] = None if w[k] is None else w[k][j0 * n:j1 * n].copy()
    for k in ('ctrl_of', 'jstate', 'lights', 'calls'):
        out[k] = w[k][j0:j1].copy()
    return words(**out)
