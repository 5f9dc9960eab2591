"""Stop signs (mpcx_stopsign: an agent of a signed movement comes to a standstill at its stop line, the stopped agents leave in the order in
which they stopped, and in the two-way case a stopped agent also waits for a gap in the unsigned road) for the tests: a plain-Python
restatement of the rule's seven steps that shares no code with the header, the host build of csrc/mpcx_stopsign_core.h
(tests/stopsign_ref/stopsign_ref.cpp) behind numpy arrays, the tables and the seeded random junctions both test files run, and the
hand-made junctions of tests/test_stopsign_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from mpc_for_av_at_intersection_amd import _lib
from tests import signal_helpers as G

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'stopsign_ref', 'stopsign_ref.cpp')
INC = G.INC
INF = float('inf')
NAN = float('nan')
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

I32_AGENT = ('path_off', 'path_len', 'traj_idx', 'cut_len', 'stopped_at', 'go', 'stopping', 'blocker')
I32_POINT = ('path_stop', 'path_move', 'path_exit')
I32_MOVE = ('conflict', 'lane', 'sign')
I32_JUNCTION = ('clock', 'ran', 'occupied', 'n_waiting')
SCALARS = ('dl', 'v_stop', 'brake', 'v_floor', 'zone', 'detect', 'patience', 'n_per')
STATE_KEYS = ('stopped_at', 'go', 'stopping', 'clock', 'ran')            # in-out
OUT_KEYS = ('cut_len',) + STATE_KEYS + ('lag', 'blocker', 'occupied', 'n_waiting')
PER_AGENT = ('state', 'done') + I32_AGENT + ('lag',)


# ---------------------------------------------------------------- the rule restated
def _where(w, q):
    """step 2's test for agent q: ('out' | 'inside' | 'approach', m, s, ti) -- the keep-clear stage's classification on the stage's tables"""
    if w.get('done') is not None and w['done'][q] != 0:
        return 'out', 0, 0, 0
    ti = int(w['traj_idx'][q])
    i = int(w['path_off'][q]) + ti
    if i < 0 or i >= len(w['path_stop']):
        return 'out', 0, 0, 0
    s, m, e = int(w['path_stop'][i]), int(w['path_move'][i]), int(w['path_exit'][i])
    if e < 0 or e > int(w['path_len'][q]) or ti >= e or m < 0 or m >= len(w['conflict']):
        return 'out', 0, 0, 0
    if s < 0 or ti >= s:
        return 'inside', m, s, ti
    if s >= int(w['path_len'][q]):
        return 'out', 0, 0, 0
    return 'approach', m, s, ti


def rule_python(w, backwards=False, log=None):
    """the seven steps restated on a dict of numpy arrays (words()), in place on OUT_KEYS; returns the agents waiting.  log: a dict that
    counts what happened (COUNTS)"""
    n_per, J = int(w['n_per']), len(w['clock'])
    dl, v_stop, brake, v_floor = (np.float64(w[k]) for k in ('dl', 'v_stop', 'brake', 'v_floor'))
    zone, detect, patience = int(w['zone']), int(w['detect']), int(w['patience'])
    conflict, lane, sign = ([int(v) & 0xffffffff for v in w[k]] for k in ('conflict', 'lane', 'sign'))
    count = (lambda k: None) if log is None else (lambda k: log.__setitem__(k, log.get(k, 0) + 1))
    total = 0
    with np.errstate(all='ignore'):
        for j in (range(J - 1, -1, -1) if backwards else range(J)):
            agents = list(range(j * n_per, (j + 1) * n_per))
            t = max(int(w['clock'][j]), 0)                                       # 1.
            new_clock = t + 1 if t < INT32_MAX else INT32_MIN
            new = {}
            occ, ran = 0, 0
            unsigned, requesters = [], []
            for q in agents:                                                    # 2.
                kind, m, s, ti = _where(w, q)
                go, st, stopping0, v = int(w['go'][q]), int(w['stopped_at'][q]), int(w['stopping'][q]), np.float64(w['state'][q, 2])
                d = s - ti
                a = dict(go=0, st=-1, stopping=0, m=m, s=s, d=d, v=v, subject=False, was=stopping0)
                if kind == 'out':
                    if w.get('done') is not None and w['done'][q] != 0 and (go != 0 or st >= 0 or stopping0 != 0):
                        count('healed')
                elif kind == 'inside':
                    occ |= 1 << m
                    if sign[m] != 0 and go == 0:
                        ran += 1
                        count('ran')
                    a.update(go=1, st=st)
                elif sign[m] == 0:
                    unsigned.append((np.float64(d) * dl / np.fmax(v, v_floor), q, m))
                elif go != 0:
                    occ |= 1 << m
                    a.update(go=go, st=st)
                elif d <= detect:
                    a.update(subject=True, st=st)
                    if st < 0 and d <= zone and v <= v_stop:
                        a['st'] = t
                        count('stamped')
                    if a['st'] >= 0:
                        requesters.append(q)
                new[q] = a
            lag = {q: (np.float64(INF), -1) for q in agents}                    # 4.
            for q in requesters:
                best = (np.float64(INF), -1)
                for eta, r, mr in unsigned:
                    if (conflict[new[q]['m']] >> mr) & 1 and (eta < best[0] or (eta == best[0] and (best[1] < 0 or r < best[1]))):
                        best = (eta, r)
                lag[q] = best
            ahead = blocked = 0                                                 # 5.
            ahead_young = 0
            by_blocked = jumped = False
            for q in sorted(requesters, key=lambda q: (new[q]['st'], q)):
                m = new[q]['m']
                why = ('occ' if conflict[m] & occ else 'blocked' if conflict[m] & blocked else 'lane' if lane[m] & ahead else
                       'gap' if not lag[q][0] >= np.float64(w['gap'][m]) else None)
                if why is None:
                    new[q]['go'] = 1
                    occ |= 1 << m
                    count('released')
                    jumped = jumped or bool(conflict[m] & ahead_young)
                else:
                    count('denied by ' + why)
                    by_blocked = by_blocked or why == 'blocked'
                    ahead |= 1 << m
                    if t - new[q]['st'] >= patience:
                        blocked |= 1 << m
                    else:
                        ahead_young |= 1 << m
            if by_blocked and jumped:
                count('aged blocks while a young one is jumped')
            waiting = 0
            for q in agents:                                                    # 6.
                a = new[q]
                if a['subject'] and a['go'] == 0:
                    can_stop = bool(np.float64(a['d']) * dl >= a['v'] * a['v'] / (np.float64(2.0) * brake))
                    if a['was'] != 0 or can_stop:
                        a['stopping'] = 1
                        if a['was'] != 0 and not can_stop:
                            count('sticky')
                    else:
                        count('exempt')
                if a['stopping'] and a['s'] < w['cut_len'][q]:
                    w['cut_len'][q] = a['s']
                w['go'][q], w['stopped_at'][q], w['stopping'][q] = a['go'], a['st'], a['stopping']
                w['lag'][q], w['blocker'][q] = lag[q]
                waiting += a['stopping']
            w['clock'][j] = new_clock                                           # 1., 7.
            w['ran'][j] = np.int32((int(w['ran'][j]) + ran + 2 ** 31) % 2 ** 32 - 2 ** 31)
            w['occupied'][j], w['n_waiting'][j] = occ, waiting
            total += waiting
    return total


COUNTS = ('stamped', 'released', 'denied by occ', 'denied by lane', 'denied by blocked', 'aged blocks while a young one is jumped', 'denied by gap',
          'sticky', 'exempt', 'ran', 'healed')


# ---------------------------------------------------------------- the host build
def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libstopsign_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.stopsign_ref_step.restype = C.c_int
    lib.stopsign_ref_step.argtypes = [C.c_int, C.c_double] + [C.c_void_p] * 6 + [C.POINTER(_lib.StopSignC), C.c_int]
    lib.stopsign_ref_layout.restype = None
    return lib


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes: per agent state (P, 4), path_off, path_len, traj_idx,
    cut_len, done (or None), stopped_at, go, stopping, lag, blocker; per path point path_stop, path_move, path_exit; per movement conflict,
    lane, sign, gap; per junction clock, ran, occupied, n_waiting; scalars dl, v_stop, brake, v_floor, zone, detect, patience, n_per"""
    w = dict(kw)
    for k in I32_AGENT + I32_POINT + I32_MOVE + I32_JUNCTION:
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    for k in ('state', 'gap', 'lag'):
        w[k] = np.ascontiguousarray(w[k], dtype=np.float64)
    w['done'] = None if w.get('done') is None else np.ascontiguousarray(w['done'], dtype=np.int32)
    assert len(w['go']) == int(w['n_per']) * len(w['clock']) and len(w['path_move']) == len(w['path_exit']) == len(w['path_stop'])
    assert len(w['conflict']) == len(w['lane']) == len(w['sign']) == len(w['gap'])
    return w


def struct_of(w, ptr):
    """the mpcx_stopsign of a dict of words; ptr: array -> address (host arrays: ctypes.data; device tensors: data_ptr())"""
    return _lib.StopSignC(*[ptr(w[k]) for k in ('path_stop', 'path_move', 'path_exit', 'conflict', 'lane', 'sign', 'gap', 'stopped_at', 'go', 'stopping',
                                                'clock', 'ran', 'lag', 'blocker', 'occupied', 'n_waiting')],
                          float(w['v_stop']), float(w['brake']), float(w['v_floor']), int(w['zone']), int(w['detect']), int(w['patience']),
                          int(w['n_per']), len(w['clock']), len(w['conflict']), len(w['path_stop']), 0)


def host_rule(lib, w, backwards=False):
    """the rule through the host build, in place on OUT_KEYS of w (a dict from words()); returns the number waiting"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    ss = struct_of(w, lambda a: a.ctypes.data)
    return lib.stopsign_ref_step(len(w['go']), float(w['dl']), p('state'), p('path_off'), p('path_len'), p('traj_idx'), p('cut_len'), p('done'),
                                 C.byref(ss), int(backwards))


def copy_words(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def same(a, b, keys=OUT_KEYS):
    """the keys on which two dicts of words differ in a byte"""
    return [k for k in keys if a[k].tobytes() != b[k].tobytes()]


# ---------------------------------------------------------------- tables and random junctions
ROUTE_LEN = 40


def route(g):
    """route g of tables(): (offset, length), its line and its exit (route-local)"""
    return (ROUTE_LEN * g, ROUTE_LEN), 10 + (3 * g) % 12, 24 + (5 * g) % 14


def tables(n_moves):
    """n_moves routes of 40 points, one per movement, and ten defective points behind them: path_stop, path_move, path_exit"""
    n = ROUTE_LEN * n_moves
    stop = np.full(n + 10, -1, np.int32); mv = np.zeros(n + 10, np.int32); ex = np.full(n + 10, -1, np.int32)
    for g in range(n_moves):
        (off, _), s, e = route(g)
        stop[off:off + s + 1] = s; mv[off:off + e] = g; ex[off:off + e] = e
    stop[n], mv[n], ex[n] = 5, n_moves + 3, 8       # a movement that does not exist
    stop[n + 1], ex[n + 1] = 12, 8                  # a line beyond the route's end (routes of 10 points start here)
    stop[n + 2], ex[n + 2] = 5, 11                  # an exit beyond the route's end
    stop[n + 3], ex[n + 3] = 6, -1                  # a line ahead without a crossing
    return stop, mv, ex


def movement_tables(rng, n_moves, signed):
    """a random symmetric conflict table without a diagonal, lanes of three consecutive movements, the sign table (signed: 'all' or
    'half': the movements of every second lane are unsigned) and gaps of 0, 2 or 3 seconds"""
    conflict = np.zeros(n_moves, np.int64)
    for g in range(n_moves):
        for h in range(g + 1, n_moves):
            if g // 3 != h // 3 and rng.random() < 0.25:
                conflict[g] |= 1 << h
                conflict[h] |= 1 << g
    lane = np.array([sum(1 << h for h in range(n_moves) if h // 3 == g // 3) for g in range(n_moves)], np.int64)
    sign = np.ones(n_moves, np.int32) if signed == 'all' else np.array([1 - (g // 3) % 2 for g in range(n_moves)], np.int32)
    return conflict.astype(np.int32), lane.astype(np.int32), sign, rng.choice([0.0, 2.0, 3.0], n_moves)


SPEEDS = (0.0, 0.0, 0.2, 0.5, 0.5000000000000001, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0, -3.0, NAN)
DL, V_STOP, BRAKE, V_FLOOR, ZONE, DETECT, PATIENCE = 0.5, 0.5, 2.0, 1.0, 4, 9, 3


def random_words(seed, n_per, n_moves, J, signed):
    """seeded random junctions: every route and the defective points, indices from before the route to behind its exit with most of them in
    the approach, speeds on both sides of v_stop, v_floor and the stopping distance (NaN among them), every value of the three state
    words, stamps on both sides of the patience, retired agents, conflict cuts on both sides of the line, clocks from negative words to
    INT32_MAX; garbage in the out words"""
    rng = np.random.default_rng([seed, n_per, n_moves, 0 if signed == 'all' else 1])
    P = n_per * J
    stop, mv, ex = tables(n_moves)
    conflict, lane, sign, gap = movement_tables(rng, n_moves, signed)
    g = rng.integers(0, n_moves, P)
    off = np.array([route(k)[0][0] for k in g]); ln = np.full(P, ROUTE_LEN)
    line = np.array([route(k)[1] for k in g])
    near = rng.random(P) < 0.93                    # most agents within the detector of their line
    ti = np.where(near, line - rng.integers(1, DETECT + 3, P), rng.integers(-2, ROUTE_LEN + 2, P))
    bad = rng.random(P) < 0.08
    off = np.where(bad, rng.choice([ROUTE_LEN * n_moves, ROUTE_LEN * n_moves + 5, -3], P), off)
    ln = np.where(bad, 10, ln)
    ti = np.where(bad, rng.integers(-2, 6, P), ti)
    state = np.zeros((P, 4)); state[:, 2] = rng.choice(SPEEDS, P)
    clock = rng.integers(0, 12, J)
    clock[rng.random(J) < 0.1] = -5
    if J > 1:
        clock[J - 1] = INT32_MAX
    t = np.repeat(np.maximum(clock, 0), n_per)
    stamp = np.where(rng.random(P) < 0.45, np.maximum(t - rng.integers(0, 7, P), 0), -1)
    return words(state=state, path_off=off, path_len=ln, traj_idx=ti, cut_len=rng.integers(5, ROUTE_LEN + 1, P), done=(rng.random(P) < 0.1).astype(int),
                 stopped_at=stamp, go=(rng.random(P) < 0.04).astype(int), stopping=(rng.random(P) < 0.4).astype(int),
                 lag=rng.random(P), blocker=rng.integers(-3, P + 3, P), path_stop=stop, path_move=mv, path_exit=ex, conflict=conflict, lane=lane,
                 sign=sign, gap=gap, clock=clock, ran=rng.integers(0, 5, J), occupied=np.full(J, -1), n_waiting=np.full(J, -1), dl=DL, v_stop=V_STOP,
                 brake=BRAKE, v_floor=V_FLOOR, zone=ZONE, detect=DETECT, patience=PATIENCE, n_per=n_per)


def drive_on(w, seed, step):
    """between two steps of a random case: most agents move on by 0 .. 2 points and change their speed, a few retire or come back"""
    rng = np.random.default_rng([seed, step, 77])
    P = len(w['go'])
    w['traj_idx'] = (w['traj_idx'] + rng.integers(0, 3, P) * (rng.random(P) < 0.6)).astype(np.int32)
    fresh = rng.random(P) < 0.5
    w['state'][fresh, 2] = rng.choice(SPEEDS, int(fresh.sum()))
    flip = rng.random(P) < 0.05
    w['done'] = np.where(flip, 1 - w['done'], w['done']).astype(np.int32)


N_PER = (1, 2, 3, 5, 8, 9, 16, 17, 33, 64)
N_MOVES = (1, 12, 16)
STEPS = 3


def group_size(n_per):
    return 1 << max(n_per - 1, 0).bit_length()


def case_set():
    """the seeded cases both test files run: (seed, n_per, n_moves, J, signed), J = 64 / G + 1 junctions so that the last wavefront of the
    kernel has dead groups"""
    out = []
    for n_per in N_PER:
        for n_moves in N_MOVES:
            for signed in ('all', 'half'):
                out.append((len(out), n_per, n_moves, 64 // group_size(n_per) + 1, signed))
    return out


# ---------------------------------------------------------------- the hand-made junctions
# Four routes of 40 points: A = movement 0, line at local index 20, exit 30; B = movement 1 (A's lane), line 20, exit 30; Cc = movement 2,
# line 10, exit 25; D = movement 3, line 15, exit 28; points 160..169 defective.  Conflicts 0 - 2, 0 - 3, 1 - 2 (conflict = 12, 4, 3, 1):
# movements 0 and 1 share a lane, the opposed straights 2 and 3 do not cross.  zone = 4 points, detect = 12, dl = 0.5 m, v_stop = 0.5 m/s,
# v_floor = 1 m/s, brake = 2 m/s^2, gap = 3 s, patience = 0.
A_, B_, C_, D_ = (0, 40), (40, 40), (80, 40), (120, 40)
H_CONFLICT, H_LANE = (12, 4, 3, 1), (3, 3, 4, 8)
ALL_WAY, TWO_WAY = (1, 1, 1, 1), (1, 1, 0, 0)       # two-way: the road of movements 2 and 3 is the through road


def hand_tables():
    stop = np.full(170, -1, np.int32); mv = np.zeros(170, np.int32); ex = np.full(170, -1, np.int32)
    for (off, _), s, e, m in ((A_, 20, 30, 0), (B_, 20, 30, 1), (C_, 10, 25, 2), (D_, 15, 28, 3)):
        stop[off:off + s + 1] = s; mv[off:off + e] = m; ex[off:off + e] = e
    stop[161], ex[161] = 12, 8                      # a line beyond the route's end
    return stop, mv, ex


def hand_words(agents, sign=ALL_WAY, clock=0, patience=0, gap=3.0):
    """one junction of `agents` = [(route, traj_idx, v)], every state word in its initial value, cut_len = the route's length"""
    stop, mv, ex = hand_tables()
    P = len(agents)
    state = np.zeros((P, 4)); state[:, 2] = [a[2] for a in agents]
    return words(state=state, path_off=[a[0][0] for a in agents], path_len=[a[0][1] for a in agents], traj_idx=[a[1] for a in agents],
                 cut_len=[a[0][1] for a in agents], done=np.zeros(P, int), stopped_at=np.full(P, -1), go=np.zeros(P, int), stopping=np.zeros(P, int),
                 lag=np.full(P, -1.0), blocker=np.full(P, -7), path_stop=stop, path_move=mv, path_exit=ex, conflict=H_CONFLICT, lane=H_LANE, sign=sign,
                 gap=np.full(4, gap), clock=[clock], ran=[0], occupied=[-1], n_waiting=[-1], dl=0.5, v_stop=0.5, brake=2.0, v_floor=1.0, zone=4,
                 detect=12, patience=patience, n_per=P)


def move_to(w, traj_idx=None, v=None):
    """the next step's inputs of a hand-made junction: new indices and speeds on last step's words"""
    if traj_idx is not None:
        w['traj_idx'] = np.ascontiguousarray(traj_idx, dtype=np.int32)
    if v is not None:
        w['state'][:, 2] = v


# ---------------------------------------------------------------- the oracle loop
class StopSignLoop:
    """The step of an oracle loop of ONE junction under stop signs, in the kernels' order: brake_helpers.BrakeOracleLoop -- the conflict
    search, the rule in the hold's place, the follower, the firm hold, the re-solve of whoever was touched -- with the stop-sign rule where
    that loop runs the priority road: for the length of a step priority_helpers.words / rule_numpy are replaced by the stop-sign words and
    `rule` (the host build: lambda w: host_rule(lib, w); or rule_python), and `stopping` travels where `yielding` does, as on the device.
    signs: dict(move, exit (per agent, route-local), conflict, lane, sign, gap, v_stop, zone, detect, v_floor, patience).  Keeps
    stopped_at, go, stopping, lag, blocker per agent and clock, ran, occupied, n_waiting; the other arguments are BrakeOracleLoop's."""

    def __init__(self, paths, dl, start, stop, group, signs, rule, brake=None, **kw):
        from tests import brake_helpers as BH
        n_moves = len(signs['conflict'])
        self.signs = dict(signs, gap=np.broadcast_to(np.asarray(signs['gap'], np.float64), (n_moves,)).copy())
        self.rule = rule
        pr = dict(move=signs['move'], exit=signs['exit'], conflict=signs['conflict'], rank=np.zeros(n_moves, np.int32), gap=0.0,
                  detect=signs['detect'], v_floor=signs['v_floor'])
        self.loop = BH.BrakeOracleLoop(paths, dl, start, stop, group, priority=pr, brake=brake, **kw)
        A = self.loop.A
        self.stopped_at, self.go, self.stopping = np.full(A, -1, np.int32), np.zeros(A, np.int32), np.zeros(A, np.int32)
        self.lag, self.blocker = np.full(A, INF), np.full(A, -1, np.int32)
        self.clock, self.ran, self.occupied, self.n_waiting = (np.zeros(1, np.int32) for _ in range(4))

    def __getattr__(self, name):        # (everything else is the inner loop's)
        return getattr(self.__dict__['loop'], name)

    def sync(self, state, applied, traj_idx, target, prev, u):
        lp = self.loop
        lp.state, lp.applied, lp.traj_idx, lp.target, lp.prev, lp.u = state, applied, traj_idx, target, prev, u

    def _words(self, **kw):
        k = self.signs
        return words(state=kw['state'], path_off=kw['path_off'], path_len=kw['path_len'], traj_idx=kw['traj_idx'], cut_len=kw['cut_len'], done=kw['done'],
                     stopped_at=self.stopped_at, go=self.go, stopping=self.stopping, lag=self.lag, blocker=self.blocker, path_stop=kw['path_stop'],
                     path_move=kw['path_move'], path_exit=kw['path_exit'], conflict=k['conflict'], lane=k['lane'], sign=k['sign'], gap=k['gap'],
                     clock=self.clock, ran=self.ran, occupied=self.occupied, n_waiting=self.n_waiting, dl=kw['dl'], v_stop=k['v_stop'],
                     brake=kw['brake'], v_floor=k['v_floor'], zone=k['zone'], detect=k['detect'], patience=k['patience'], n_per=kw['n_per'])

    def _rule(self, w):
        self.rule(w)
        self.stopped_at, self.go, self.stopping, self.lag, self.blocker = (w[k] for k in ('stopped_at', 'go', 'stopping', 'lag', 'blocker'))
        self.clock, self.ran, self.occupied, self.n_waiting = (w[k] for k in ('clock', 'ran', 'occupied', 'n_waiting'))
        w['yielding'], w['waited'] = w['stopping'].copy(), w['stopping'].copy()

    def step(self):
        from tests import priority_helpers as PH
        assert callable(getattr(PH, 'words', None)) and callable(getattr(PH, 'rule_numpy', None)), 'priority_helpers no longer has words / rule_numpy'
        keep = PH.words, PH.rule_numpy
        PH.words, PH.rule_numpy = self._words, self._rule
        clock = int(self.clock[0])
        try:
            out = self.loop.step()
        finally:
            PH.words, PH.rule_numpy = keep
        # (the inner loop really went through the two names: the rule ran once and ticked the junction's clock)
        assert int(self.clock[0]) == (clock + 1 if 0 <= clock < INT32_MAX else 1 if clock < 0 else INT32_MIN), 'BrakeOracleLoop.step did not run the rule'
        return out


STOCK_PAIRS = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2))      # stock_routes()' eight (arm, turn)


def stock_tables(route_idx):
    """(paths, dl, stop, group, move, exit, conflict, lane) of the agents on the stock routes `route_idx` (indices into stock_routes()'
    eight): stop_lines()' and movement_lines()' rows per agent, movement_conflicts() of the eight routes for the stock disc model -- the
    defaults of IntersectionBatch.stop_signs()"""
    from mpc_for_av_at_intersection_amd.batch import movement_conflicts, movement_lines, stop_lines
    from tests import helpers as H
    from tests import scene_helpers as SH
    every = [H.smoothed_path(*pr) for pr in STOCK_PAIRS]
    dl = float(np.linalg.norm(every[0][0, :2] - every[0][1, :2]))
    stop, group = stop_lines(every)
    _, move, ex = movement_lines(every)
    cd = SH.car()
    conflict, lane = movement_conflicts(every, stop, ex, np.asarray(cd.circle_centers, dtype=np.float64), float(cd.radius))
    offs = np.cumsum([0] + [len(p) for p in every])
    pick = lambda t: [t[offs[k]:offs[k + 1]] for k in route_idx]
    return [every[k] for k in route_idx], dl, pick(stop), pick(group), pick(move), pick(ex), conflict, lane


def stock_loop(route_idx, start, rule, signed=None, gap=5.0, v_stop=0.5, zone=None, patience=0, speed=False, firm=None, T=13, **kw):
    """a StopSignLoop of agents on the stock routes from the indices `start` with stop_signs()' defaults; firm: brake_helpers.BRAKE-like dict
    (brake, setback) or None"""
    from mpc_for_av_at_intersection_amd.batch import sign_table
    paths, dl, stop, group, move, ex, conflict, lane = stock_tables(route_idx)
    zone = int(np.ceil(4.0 / dl)) if zone is None else zone
    signs = dict(move=move, exit=ex, conflict=conflict, lane=lane, sign=sign_table(signed), gap=gap, v_stop=v_stop, zone=zone,
                 detect=max(max(int(s[0]) for s in stop), zone), v_floor=1.0, patience=patience)
    return StopSignLoop(paths, dl, list(start), stop, group, signs, rule, brake=firm, T=T, depart=True, speed=speed, **kw)
