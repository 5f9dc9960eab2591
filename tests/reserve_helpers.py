"""Crossing reservations (mpcx_reservation: a manager per junction admits a car only if its movement conflicts with no movement that holds
the crossing; the hold at the line is the signal rule's) for the tests: a numpy restatement of the rule, the host build of
csrc/mpcx_reserve_core.h (tests/reserve_ref/reserve_ref.cpp) behind numpy arrays, the hand-made junctions of tests/test_reserve_cpu.py and
the closed loop of several egos on the CPU oracle under the rule (ReserveOracleLoop, a subclass of signal_helpers.SignalOracleLoop in which
a conflict-search pass for all driving agents comes first, then the junction's rule, then the hold's re-solve)."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle_py as orc
from tests import helpers as H
from tests import precedence_helpers as PH
from tests import scene_helpers as SH
from tests import signal_helpers as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'reserve_ref', 'reserve_ref.cpp')
INC = G.INC
UNBOUNDED = int(np.iinfo(np.int32).max)


# ---------------------------------------------------------------- the rule restated
def classify(w, q):
    """step 2's test for agent q: ('out' | 'inside' | 'approach', g, s - ti)"""
    if w.get('done') is not None and w['done'][q]:
        return 'out', 0, 0
    ti = int(w['traj_idx'][q])
    i = int(w['path_off'][q]) + ti
    if not 0 <= i < len(w['path_stop']):
        return 'out', 0, 0
    s, g, e = int(w['path_stop'][i]), int(w['path_group'][i]), int(w['path_exit'][i])
    if e < 0 or e > int(w['path_len'][q]) or ti >= e or not 0 <= g < int(w['n_groups']):
        return 'out', 0, 0
    if s < 0 or ti >= s:
        return 'inside', g, 0
    if s >= int(w['path_len'][q]):
        return 'out', 0, 0
    return 'approach', g, s - ti


def rule_numpy(w, backwards=False, log=None, refused=None):
    """the rule restated on a dict of numpy arrays (words()), in place on grant, since, clock, occupied, queued, held and cut_len; returns
    the agents held.  log: a list that receives (junction, agent, movement, occ before the grant) for every grant given; refused: a list
    that receives (junction, agent, movement, occ, blocked, ahead) as they stood for every request denied"""
    n_per, J = int(w['n_per']), len(w['mgr_of'])
    n_mgr = len(w['mgr_time'])
    got = 0
    for j in (range(J - 1, -1, -1) if backwards else range(J)):
        k = int(w['mgr_of'][j])
        agents = list(range(j * n_per, (j + 1) * n_per))
        if not 0 <= k < n_mgr:
            w['occupied'][j] = w['queued'][j] = 0
            for q in agents:
                w['held'][q] = 0
            continue
        t = max(int(w['clock'][j]), 0)
        w['clock'][j] = np.array(t + 1, dtype=np.int64).astype(np.int32)        # (wraps at 2^31)
        detect, patience = int(w['mgr_time'][k][0]), int(w['mgr_time'][k][1])
        occ, requests, kinds = 0, [], {}
        for m, q in enumerate(agents):
            kind, g, d = kinds[q] = classify(w, q)
            if kind == 'out':
                w['grant'][q], w['since'][q] = 0, -1
            elif kind == 'inside':
                w['grant'][q] = 1
                occ |= 1 << g
            elif w['grant'][q] != 0:
                occ |= 1 << g
            elif d <= detect:
                if w['since'][q] < 0:
                    w['since'][q] = t
                requests.append((int(w['since'][q]), min(d, 65535), m, g, q))
            else:
                w['since'][q] = -1
        ahead = blocked = denied = 0
        for since, _, _, g, q in sorted(requests):
            if int(w['conflict'][g]) & (occ | blocked) == 0 and int(w['lane'][g]) & ahead == 0:
                if log is not None:
                    log.append((j, q, g, occ))
                w['grant'][q] = 1
                occ |= 1 << g
            else:
                if refused is not None:
                    refused.append((j, q, g, occ, blocked, ahead))
                ahead |= 1 << g
                denied += 1
                if t - since >= patience:
                    blocked |= 1 << g
        w['occupied'][j], w['queued'][j] = occ, denied
        for q in agents:
            kind, g, d = kinds[q]
            held = 0
            if kind == 'approach' and w['grant'][q] == 0:
                held = 1
                s = int(w['traj_idx'][q]) + d
                if s < w['cut_len'][q]:
                    w['cut_len'][q] = s
            w['held'][q] = held
            got += held
    return got


# ---------------------------------------------------------------- the host build
def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libreserve_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.reserve_ref_step.restype = C.c_int
    lib.reserve_ref_step.argtypes = ([C.c_int, C.c_double] + [C.c_void_p] * 9 + [C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_int] * 4)
    lib.reserve_ref_layout.restype = None
    return lib


I32_KEYS = ('path_off', 'path_len', 'traj_idx', 'cut_len', 'path_stop', 'path_group', 'path_exit', 'held', 'conflict', 'lane', 'mgr_time', 'mgr_of',
            'grant', 'since', 'clock', 'occupied', 'queued')
OUT_KEYS = ('grant', 'since', 'clock', 'occupied', 'queued', 'held', 'cut_len')
PER_AGENT = ('state', 'path_off', 'path_len', 'traj_idx', 'cut_len', 'held', 'done', 'grant', 'since')
PER_JUNCTION = ('mgr_of', 'clock', 'occupied', 'queued')


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes: per agent state (P, 4), path_off, path_len, traj_idx,
    cut_len, done (or None), held, grant, since; per path point path_stop, path_group, path_exit; per movement conflict, lane; mgr_time
    (n_mgr, 2); per junction mgr_of, clock, occupied, queued; scalars dl, brake, n_groups, n_per"""
    w = dict(kw)
    for k in I32_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    w['state'] = np.ascontiguousarray(w['state'], dtype=np.float64)
    w['done'] = None if w.get('done') is None else np.ascontiguousarray(w['done'], dtype=np.int32)
    assert w['mgr_time'].ndim == 2 and len(w['held']) == int(w['n_per']) * len(w['mgr_of']) and len(w['conflict']) == len(w['lane']) == int(w['n_groups'])
    return w


def host_rule(lib, w, backwards=False):
    """the rule through the host build, in place on OUT_KEYS of w (a dict from words()); returns the number held"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    return lib.reserve_ref_step(len(w['held']), float(w['dl']), p('state'), p('path_off'), p('path_len'), p('traj_idx'), p('cut_len'), p('done'),
                                p('path_stop'), p('path_group'), p('held'), float(w['brake']), len(w['path_stop']), int(w['n_groups']),
                                p('path_exit'), p('conflict'), p('lane'), p('mgr_time'), p('mgr_of'), p('grant'), p('since'), p('clock'),
                                p('occupied'), p('queued'), int(w['n_per']), len(w['mgr_of']), len(w['mgr_time']), int(backwards))


def copy_words(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def blob(w, backwards):
    """a case of the stand-alone program's input file"""
    b = np.array([len(w['held']), len(w['path_stop']), w['n_groups'], w['n_per'], len(w['mgr_of']), len(w['mgr_time']), int(w['done'] is not None),
                  int(backwards)], np.int32).tobytes()
    b += np.array([w['dl'], w['brake']], np.float64).tobytes() + w['state'].tobytes()
    for k in ('path_off', 'path_len', 'traj_idx', 'cut_len'):
        b += w[k].tobytes()
    if w['done'] is not None:
        b += w['done'].tobytes()
    for k in ('path_stop', 'path_group', 'path_exit', 'held', 'conflict', 'lane', 'mgr_time', 'mgr_of', 'grant', 'since', 'clock', 'occupied', 'queued'):
        b += w[k].tobytes()
    return b


def out_bytes(w, got):
    """what the stand-alone program writes for a case"""
    return b''.join(w[k].tobytes() for k in OUT_KEYS) + np.array([got], np.int32).tobytes()


def junctions(w, j0, j1):
    """the words of junctions [j0, j1) alone (the tables stay whole)"""
    n = int(w['n_per'])
    out = dict(w)
    for k in PER_AGENT:
        out[k] = None if w[k] is None else w[k][j0 * n:j1 * n].copy()
    for k in PER_JUNCTION:
        out[k] = w[k][j0:j1].copy()
    return words(**out)


# ---------------------------------------------------------------- the hand-made junctions
# Four routes of 40 points in a table of 170: A = points 0..39, line at local index 20, exit 30, movement 0; B = 40..79, line 20, exit 30,
# movement 1 (A's approach lane); Cc = 80..119, line 10, exit 25, movement 2; D = 120..159, line 15, exit 28, movement 3.  Conflicts: 0 - 2,
# 0 - 3, 1 - 3 (conflict = 12, 8, 1, 3); lanes: {0, 1}, {2}, {3} (lane = 3, 3, 4, 8).  Points 160..169 are defective (below).  Two managers,
# both with detect 8 points: manager 0 has patience 0, manager 1 patience 5.
A_, B_, C_, D_ = (0, 40), (40, 40), (80, 40), (120, 40)
DEF = (160, 10)
CONFLICT, LANE, MGR_TIME = (12, 8, 1, 3), (3, 3, 4, 8), ((8, 0), (8, 5))
PAD = (D_, 30, 40, 0, -1, 0, 0)     # (route, traj_idx, cut, grant, since, held, done): past its exit -- OUT, never held (fills a junction)
BIG = UNBOUNDED

CASES = [
    # (what, manager, clock as read, agents) -> want (clock, occupied, queued, [(grant, since, held, cut) per agent])
    ('a lone requester', 0, 7, [(A_, 15, 40, 0, -1, 1, 0)], (8, 1, 0, [(1, 7, 0, 40)])),
    ('equal since: the nearer car (4 points against 5) goes first', 0, 9, [(A_, 15, 40, 0, 3, 1, 0), (C_, 6, 40, 0, 3, 1, 0)],
     (10, 4, 1, [(0, 3, 1, 20), (1, 3, 0, 40)])),
    ('equal since and distance: the lower index goes first', 0, 9, [(A_, 15, 40, 0, 3, 0, 0), (C_, 5, 40, 0, 3, 0, 0)],
     (10, 1, 1, [(1, 3, 0, 40), (0, 3, 1, 10)])),
    ('an aged denied requester blocks a later one compatible with occ; a conflict cut below the line is kept', 1, 20,
     [(D_, 20, 40, 1, -1, 0, 0), (A_, 15, 40, 0, 10, 1, 0), (C_, 5, 8, 0, 15, 1, 0)], (21, 8, 2, [(1, -1, 0, 40), (0, 10, 1, 20), (0, 15, 1, 8)])),
    ('the same pair not yet aged: the later one passes', 1, 20, [(D_, 20, 40, 1, -1, 0, 0), (A_, 15, 40, 0, 17, 1, 0), (C_, 5, 40, 0, 18, 1, 0)],
     (21, 12, 1, [(1, -1, 0, 40), (0, 17, 1, 20), (1, 18, 0, 40)])),
    ('the lane rule: the rear car of movement 1 behind a denied front car of movement 0', 1, 20,
     [(C_, 12, 40, 1, -1, 0, 0), (A_, 18, 40, 0, 17, 1, 0), (B_, 12, 40, 0, 18, 0, 0)], (21, 4, 2, [(1, -1, 0, 40), (0, 17, 1, 20), (0, 18, 1, 20)])),
    ('a sticky grant with a conflicting car INSIDE', 0, 5, [(A_, 15, 40, 1, 4, 0, 0), (C_, 12, 40, 1, -1, 0, 0)], (6, 5, 0, [(1, 4, 0, 40), (1, -1, 0, 40)])),
    ('an INSIDE agent without a grant', 0, 5, [(D_, 20, 40, 0, -1, 1, 0)], (6, 8, 0, [(1, -1, 0, 40)])),
    ('ON the line counts as INSIDE; since is left alone', 0, 5, [(A_, 20, 40, 0, 6, 1, 0)], (6, 1, 0, [(1, 6, 0, 40)])),
    ('release at ti == e, the waiting conflicting car granted in the same step', 0, 30, [(C_, 25, 40, 1, 2, 0, 0), (A_, 19, 40, 0, 5, 1, 0)],
     (31, 1, 0, [(0, -1, 0, 40), (1, 5, 0, 40)])),
    ('one point before the exit still holds the crossing', 0, 30, [(C_, 24, 40, 1, 2, 0, 0), (A_, 19, 40, 0, 5, 1, 0)],
     (31, 4, 1, [(1, 2, 0, 40), (0, 5, 1, 20)])),
    ('beyond the detector (9 > 8): held, a stale since goes to -1', 0, 5, [(A_, 11, 40, 0, 6, 0, 0)], (6, 0, 0, [(0, -1, 1, 20)])),
    ('s - traj_idx = 8 = detect requests', 0, 5, [(A_, 12, 40, 0, -1, 1, 0)], (6, 1, 0, [(1, 5, 0, 40)])),
    ('a done agent that holds a grant gives it back: the conflicting car is granted', 0, 12, [(A_, 15, 40, 1, 3, 1, 1), (C_, 6, 40, 0, -1, 1, 0)],
     (13, 4, 0, [(0, -1, 0, 40), (1, 12, 0, 40)])),
    ('defective point: movement 7 of 4', 0, 5, [(DEF, 0, 10, 1, 3, 1, 0)], (6, 0, 0, [(0, -1, 0, 10)])),
    ('defective point: s = 12 >= path_len = 10', 0, 5, [(DEF, 1, 10, 1, 3, 1, 0)], (6, 0, 0, [(0, -1, 0, 10)])),
    ('defective point: e = 11 > path_len = 10', 0, 5, [(DEF, 2, 10, 1, 3, 1, 0)], (6, 0, 0, [(0, -1, 0, 10)])),
    ('defective point: a line ahead and e = -1: free', 0, 5, [(DEF, 3, 10, 1, 3, 1, 0)], (6, 0, 0, [(0, -1, 0, 10)])),
    ('defective index: i = 173 outside [0, 170); i = -4', 0, 5, [((168, 10), 5, 10, 1, 3, 1, 0), ((-9, 10), 5, 10, 1, 3, 1, 0)],
     (6, 0, 0, [(0, -1, 0, 10), (0, -1, 0, 10)])),
    ('a negative clock counts as 0', 0, -5, [(A_, 15, 40, 0, -1, 0, 0)], (1, 1, 0, [(1, 0, 0, 40)])),
    ('the clock wraps at 2^31 - 1', 1, BIG, [(A_, 15, 40, 0, -1, 0, 0)], (-BIG - 1, 1, 0, [(1, BIG, 0, 40)])),
    ('mgr_of = 2 of 2: no manager, the words left alone, a hold dropped', 2, 9, [(A_, 15, 12, 1, 3, 1, 0)], (9, 0, 0, [(1, 3, 0, 12)])),
    ('mgr_of = -1', -1, -7, [(A_, 15, 40, 0, -1, 1, 0)], (-7, 0, 0, [(0, -1, 0, 40)])),
    ('an empty junction', 0, 3, [], (4, 0, 0, [])),
]

# junctions of 64 (n_per = 64 only): (what, manager, clock, [(slot, agent)] or a callable slot -> agent) -> want as above per slot
WIDE = [
    ('64 requesters of one movement: all granted', 0, 2, lambda m: (A_, 15, 40, 0, -1, 1, 0), (3, 1, 0, lambda m: (1, 2, 0, 40))),
    ('63 requesters behind a conflicting car INSIDE: all denied', 0, 2, lambda m: (C_, 12, 40, 0, -1, 0, 0) if m == 17 else (A_, 15, 40, 0, -1, 0, 0),
     (3, 4, 63, lambda m: (1, -1, 0, 40) if m == 17 else (0, 2, 1, 20))),
    ('movements 0 and 2 alternating, equal since and distance: the first lane wins, 63 denied', 0, 2,
     lambda m: (C_, 5, 40, 0, -1, 0, 0) if m & 1 else (A_, 15, 40, 0, -1, 0, 0),
     (3, 1, 63, lambda m: (1, 2, 0, 40) if m == 0 else (0, 2, 1, 10) if m & 1 else (0, 2, 1, 20))),
]


def _tables():
    stop = np.full(170, -1, np.int32); grp = np.zeros(170, np.int32); ex = np.full(170, -1, np.int32)
    for (off, _), s, e, g in ((A_, 20, 30, 0), (B_, 20, 30, 1), (C_, 10, 25, 2), (D_, 15, 28, 3)):
        stop[off:off + s + 1] = s; grp[off:off + e] = g; ex[off:off + e] = e
    stop[160], grp[160], ex[160] = 5, 7, 8          # a movement that does not exist
    stop[161], ex[161] = 12, 8                      # a line beyond the route's end
    stop[162], ex[162] = 5, 11                      # an exit beyond the route's end
    stop[163], ex[163] = 6, -1                      # a line ahead without a crossing
    return stop, grp, ex


def slots(n_agents, n_per):
    """where a case's agents sit in a junction of n_per, in ascending order (the index decides ties): spread from the first slot to the last"""
    return [n_per - 1] if n_agents == 1 else [int(round(v)) for v in np.linspace(0, n_per - 1, n_agents)]


def hand_made(n_per, repeat=1):
    """CASES as junctions of n_per agents (the cases with more agents than n_per are left out), `repeat` times over, at n_per = 64 followed
    by WIDE; returns (words, want) with want = (clock (J,), occupied (J,), queued (J,), {agent: (grant, since, held, cut)})"""
    stop, grp, ex = _tables()
    cases = [c for c in CASES if len(c[3]) <= n_per] * repeat
    rows, want_agent, head = [], {}, []
    for j, (_, mgr, clock, agents, want) in enumerate(cases):
        rows += [PAD] * n_per
        for slot, ag, wa in zip(slots(len(agents), n_per), agents, want[3]):
            rows[j * n_per + slot] = ag
            want_agent[j * n_per + slot] = wa
        head.append((mgr, clock) + tuple(want[:3]))
    if n_per == 64:
        for _, mgr, clock, agent_at, want in WIDE:
            base = len(rows)
            rows += [agent_at(m) for m in range(64)]
            want_agent.update({base + m: want[3](m) for m in range(64)})
            head.append((mgr, clock) + tuple(want[:3]))
    P, J = len(rows), len(head)
    col = lambda k: [r[k] for r in rows]
    w = words(state=np.zeros((P, 4)), path_off=[r[0][0] for r in rows], path_len=[r[0][1] for r in rows], traj_idx=col(1), cut_len=col(2),
              grant=col(3), since=col(4), held=col(5), done=col(6), path_stop=stop, path_group=grp, path_exit=ex, conflict=CONFLICT, lane=LANE,
              mgr_time=MGR_TIME, mgr_of=[h[0] for h in head], clock=np.array([h[1] for h in head], dtype=np.int64), occupied=np.full(J, -1),
              queued=np.full(J, -1), dl=0.5, brake=2.0, n_groups=4, n_per=n_per)
    want = (np.array([h[2] for h in head], np.int64).astype(np.int32), np.array([h[3] for h in head], np.int32),
            np.array([h[4] for h in head], np.int32), want_agent)
    return w, want


def check_against_want(w, want, rows):
    """the words after the rule against the hand-written expectations; rows: the words before"""
    ck, oc, qu, ag = want
    assert np.array_equal(w['clock'], ck), np.flatnonzero(w['clock'] != ck)
    assert np.array_equal(w['occupied'], oc), np.flatnonzero(w['occupied'] != oc)
    assert np.array_equal(w['queued'], qu), np.flatnonzero(w['queued'] != qu)
    for q in range(len(w['held'])):
        exp = ag.get(q, (0, -1, 0, int(rows['cut_len'][q])))      # (a padding agent is OUT: no grant, never held, its cut kept)
        got = (int(w['grant'][q]), int(w['since'][q]), int(w['held'][q]), int(w['cut_len'][q]))
        assert got == exp, (q, got, exp)


# ---------------------------------------------------------------- the oracle loop
HALF_WIDTH = G.HALF_WIDTH


class ReserveOracleLoop(G.SignalOracleLoop):
    """SignalOracleLoop with ONE junction's manager in the place of the clock, cut mode.  stop, group, exit: per agent, the route-local
    tables of its path (movement_lines()' rows of its route); conflict, lane: movement_conflicts()' words.  A step is a conflict-search
    pass (orc.agent_step) for all driving agents, then the junction's rule (rule_numpy) on the traj_idx those returned -- the kernel's
    order: the stage runs behind the conflict search --, then, for a held agent whose line lies below the returned cut, the window, rollout
    and QP again on full[:s].  Records per step occupied and queued, every grant with the occ before it (grants: (step, agent, movement,
    occ)), the steps at whose start cars of conflicting movements were inside the crossing square together (mixed_steps) and the true
    clearance."""

    def __init__(self, paths, dl, start, stop, group, exit, conflict, lane, detect, patience, **kw):
        n_groups = len(conflict)
        super().__init__(paths, dl, start, stop, group, dict(cycle=1, amber=0, green=[[k, 0] for k in range(n_groups)]), **kw)
        assert not self.speed
        offs = np.cumsum([0] + [len(p) for p in paths])
        self.tab = dict(path_stop=np.concatenate(stop), path_group=np.concatenate(group), path_exit=np.concatenate(exit), conflict=conflict,
                        lane=lane, mgr_time=[[int(detect), UNBOUNDED if patience is None else int(patience)]], mgr_of=[0], dl=self.dl,
                        brake=self.brake, n_groups=n_groups, n_per=self.A, path_off=offs[:-1], path_len=[len(p) for p in paths])
        self.movement = [int(np.asarray(g)[0]) for g in group]
        self.grant, self.since, self.clock = np.zeros(self.A, np.int32), np.full(self.A, -1, np.int32), np.zeros(1, np.int32)
        self.occupied_hist, self.queued_hist, self.grants = [], [], []

    def _measure(self, pool):
        live = [a for a in range(self.A) if not self.done[a] and not self.absent[a]]
        for a in live:
            others = [r for r in live if r != a]
            if others:
                self.worst_clearance = min(self.worst_clearance, SH.clearance(pool, a, others, self.centers, self.radius))
        inside = [a for a in live if max(abs(pool[a, 0]), abs(pool[a, 1])) <= HALF_WIDTH]
        if any((int(self.tab['conflict'][self.movement[a]]) >> self.movement[b]) & 1 for a in inside for b in inside):
            self.mixed_steps.append(self.steps)

    def step(self):
        A = self.A
        pool = self.pool()
        self._measure(pool)
        gone = list(self.absent) + [False] * (len(pool) - A)
        res, present = [None] * A, [None] * A
        for a in range(A):          # the conflict search (and, for whoever is not held, the whole step) of every driving agent
            if self.done[a]:
                continue
            present[a] = [r for r in range(len(pool)) if r != a and not gone[r]]
            res[a] = orc.agent_step(self.p, np.ascontiguousarray(self.paths[a], np.float64), self.dl, self.state[a], pool[present[a]],
                                    self.traj_idx[a], self.prev[a], self.target[a], self.u[a], self.centers, self.radius, self.margin)
        drive = [r is not None for r in res]
        w = words(state=self.state, traj_idx=[int(res[a]['traj_idx']) if drive[a] else self.traj_idx[a] for a in range(A)],
                  cut_len=[int(res[a]['cut']) if drive[a] else 0 for a in range(A)], done=[0 if d else 1 for d in drive], held=self.held,
                  grant=self.grant, since=self.since, clock=self.clock, occupied=[0], queued=[0], **self.tab)
        log = []
        rule_numpy(w, log=log)
        self.grant, self.since, self.clock, self.held = w['grant'], w['since'], w['clock'], [int(h) for h in w['held']]
        self.occupied_hist.append(int(w['occupied'][0])); self.queued_hist.append(int(w['queued'][0]))
        self.grants += [(self.steps, q, g, occ) for _, q, g, occ in log]
        out = [None] * A
        new_state, new_applied = self.state.copy(), self.applied.copy()
        arrived = []
        for a in range(A):
            if not drive[a]:
                continue
            r, full, st = res[a], np.ascontiguousarray(self.paths[a], np.float64), self.state[a]
            cut, sol, target, held = int(r['cut']), r['sol'], r['target_ind'], self.held[a]
            s = int(w['cut_len'][a])
            if held and s < cut:        # the hold's re-solve: window, rollout and QP on full[:s], with the pieces agent_step itself calls
                cut = s
                uw = np.zeros((2, self.p.T)) if self.u[a] is None else np.asarray(self.u[a], float)
                tmp = full[:s]
                xref, target, re = orc.calc_ref_trajectory(self.p, st, tmp[:, 0], tmp[:, 1], tmp[:, 2], self.dl, self.target[a])
                assert target >= 0
                xbar = orc.predict_motion(self.p, list(st), uw[0], uw[1])
                sol = orc.qp_solve(self.p, list(st), xref, xbar, re, uw)
            assert sol.status == 0, (self.steps, a, sol.status)
            post = np.asarray(orc.plant_step(self.p, st, sol.u[0, 0], sol.u[1, 0]), dtype=np.float64)
            self.traj_idx[a], self.target[a], self.prev[a], self.u[a] = int(r['traj_idx']), int(target), int(cut), sol.u.copy()
            new_state[a] = post
            new_applied[a] = (sol.u[1, 0], sol.u[0, 0])
            out[a] = dict(pool=pool, present=present[a], hit=-1 if r['hit'] is None else int(r['hit'][2]), cut=int(cut), goal_len=int(cut),
                          target=int(target), traj_idx=int(r['traj_idx']), x_sol=sol.x.copy(), u_sol=sol.u.copy(), post=post.copy(),
                          ctrl=new_applied[a].copy(), status=int(sol.status), held=int(held), grant=int(self.grant[a]), since=int(self.since[a]))
            if SH.is_goal(post, full[-1], target, cut):
                arrived.append(a)
        self.state, self.applied = new_state, new_applied
        self.steps += 1
        for a in arrived:
            self.done[a], self.arrival[a] = True, self.steps
            self.applied[a] = 0.0
            if self.depart:
                self.absent[a] = True
        return out


def scene_tables(name):
    """(paths, dl, start, stop, group, exit, conflict, lane) of precedence_helpers' scenes 'straight', 'turn1' and 'eight' with the
    movement tables of batch.movement_lines() / movement_conflicts() for the stock disc model"""
    from mpc_for_av_at_intersection_amd.batch import movement_conflicts, movement_lines
    pairs, start = PH.scene(name)
    paths = [H.smoothed_path(*pr) for pr in pairs]
    dl = float(np.linalg.norm(paths[0][0, :2] - paths[0][1, :2]))
    stop, group, ex = movement_lines(paths)
    cd = SH.car()
    conflict, lane = movement_conflicts(paths, stop, ex, np.asarray(cd.circle_centers, dtype=np.float64), float(cd.radius))
    offs = np.cumsum([0] + [len(p) for p in paths])
    split = lambda t: [t[offs[k]:offs[k + 1]] for k in range(len(paths))]
    return paths, dl, start, split(stop), split(group), split(ex), conflict, lane


def scene_loop(name, patience, detect=None):
    """the scene under a manager whose detector is the whole approach (T = 13, v0 = 0, cut mode, departure on)"""
    paths, dl, start, stop, group, ex, conflict, lane = scene_tables(name)
    detect = max(int(s[0]) for s in stop) if detect is None else detect
    return ReserveOracleLoop(paths, dl, start, stop, group, ex, conflict, lane, detect, patience, T=13, depart=True)
