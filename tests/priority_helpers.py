"""Priority road (mpcx_priority: an agent of a minor movement waits at its stop line until the conflicting movements of smaller rank leave
it a gap) for the tests: a numpy restatement of the rule, the host build of csrc/mpcx_priority_core.h
(tests/priority_ref/priority_ref.cpp) behind numpy arrays, the hand-made junctions of tests/test_priority_cpu.py, seeded random words,
and the closed loop of several egos on the CPU oracle under the rule: PriorityLoop -- one junction, no lights, a conflict-search pass for
all driving agents first, then the rule, then the re-solve of whoever was cut -- and the two scenes both test files run."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle_py as orc
from tests import helpers as H
from tests import keepclear_helpers as KH
from tests import scene_helpers as SH
from tests import signal_helpers as G

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'priority_ref', 'priority_ref.cpp')
INC = G.INC
INF = float('inf')


# ---------------------------------------------------------------- the rule restated
def eta_of(w, q, kind, s, ti):
    """step 2: seconds until agent q is at its line at its present speed, 0.0 inside"""
    if kind == 'inside':
        return np.float64(0.0)
    return np.float64(s - ti) * np.float64(w['dl']) / np.fmax(np.float64(w['state'][q, 2]), np.float64(w['v_floor']))


def meet(w, kinds, q, m, agents):
    """step 3 for an agent q of movement m among `agents`: (lag, blocker), the lexicographic minimum of (eta, index) over the others that
    are not OUT, have a smaller rank and conflict with m; (+inf, -1) if there is none"""
    lag, blocker = np.float64(INF), -1
    for r in agents:
        kind, mr, sr, tr = kinds[r]
        if r == q or kind == 'out' or not int(w['rank'][mr]) < int(w['rank'][m]) or not (int(w['conflict'][m]) >> mr) & 1:
            continue
        eta = eta_of(w, r, kind, sr, tr)
        if eta < lag or (eta == lag and (blocker < 0 or r < blocker)):
            lag, blocker = eta, r
    return lag, blocker


def rule_numpy(w, backwards=False, log=None):
    """the rule restated on a dict of numpy arrays (words()), in place on cut_len, waited, yielding, blocker, lag, occupied and n_yielding;
    returns the agents yielding.  log: a list that receives (junction, agent, movement, blocker, lag, why) for every THREATENED candidate,
    why = 'waited', 'can stop' or 'exempt' (it cannot stop any more and is left free)"""
    n_per, J = int(w['n_per']), len(w['occupied'])
    detect = int(w['detect'])
    got = 0
    with np.errstate(all='ignore'):
        for j in (range(J - 1, -1, -1) if backwards else range(J)):
            agents = list(range(j * n_per, (j + 1) * n_per))
            kinds = {q: KH.classify(w, q) for q in agents}
            occ = 0
            for q in agents:
                if kinds[q][0] == 'inside':
                    occ |= 1 << kinds[q][1]
            res = {}
            for q in agents:        # everything is read before anything is written
                kind, m, s, ti = kinds[q]
                lag, blocker, yielding = np.float64(INF), -1, 0
                if kind == 'approach' and s - ti <= detect:
                    lag, blocker = meet(w, kinds, q, m, agents)
                    if lag < np.float64(w['gap'][m]):
                        v = np.float64(w['state'][q, 2])
                        if w['waited'][q] != 0:
                            yielding, why = 1, 'waited'
                        elif np.float64(s - ti) * np.float64(w['dl']) >= v * v / (np.float64(2.0) * np.float64(w['brake'])):
                            yielding, why = 1, 'can stop'
                        else:
                            why = 'exempt'
                        if log is not None:
                            log.append((j, q, m, blocker, float(lag), why))
                res[q] = (lag, blocker, yielding, s)
            n = 0
            for q in agents:
                lag, blocker, yielding, s = res[q]
                if yielding and s < w['cut_len'][q]:
                    w['cut_len'][q] = s
                w['lag'][q], w['blocker'][q], w['yielding'][q], w['waited'][q] = lag, blocker, yielding, yielding
                n += yielding
            w['occupied'][j], w['n_yielding'][j] = occ, n
            got += n
    return got


# ---------------------------------------------------------------- the host build
def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libpriority_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.priority_ref_step.restype = C.c_int
    lib.priority_ref_step.argtypes = [C.c_int, C.c_double] + [C.c_void_p] * 18 + [C.c_double, C.c_double] + [C.c_int] * 6
    lib.priority_ref_layout.restype = None
    return lib


I32_KEYS = ('path_off', 'path_len', 'traj_idx', 'cut_len', 'path_stop', 'path_move', 'path_exit', 'conflict', 'rank', 'waited', 'yielding', 'blocker',
            'occupied', 'n_yielding')
F64_KEYS = ('state', 'gap', 'lag')
OUT_KEYS = ('cut_len', 'waited', 'yielding', 'blocker', 'lag', 'occupied', 'n_yielding')
PER_AGENT = ('state', 'path_off', 'path_len', 'traj_idx', 'cut_len', 'done', 'waited', 'yielding', 'blocker', 'lag')
PER_JUNCTION = ('occupied', 'n_yielding')


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes: per agent state (P, 4), path_off, path_len, traj_idx,
    cut_len, done (or None), waited, yielding, blocker, lag; per path point path_stop, path_move, path_exit; per movement conflict, rank,
    gap; per junction occupied, n_yielding; scalars dl, v_floor, brake, detect, n_per"""
    w = dict(kw)
    for k in I32_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    for k in F64_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.float64)
    w['done'] = None if w.get('done') is None else np.ascontiguousarray(w['done'], dtype=np.int32)
    assert len(w['waited']) == int(w['n_per']) * len(w['occupied']) and len(w['path_move']) == len(w['path_exit']) == len(w['path_stop'])
    assert len(w['conflict']) == len(w['rank']) == len(w['gap'])
    return w


def host_rule(lib, w, backwards=False):
    """the rule through the host build, in place on OUT_KEYS of w (a dict from words()); returns the number yielding"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    return lib.priority_ref_step(len(w['waited']), float(w['dl']), p('state'), p('path_off'), p('path_len'), p('traj_idx'), p('cut_len'), p('done'),
                                 p('path_stop'), p('path_move'), p('path_exit'), p('conflict'), p('rank'), p('gap'), p('waited'), p('yielding'),
                                 p('blocker'), p('lag'), p('occupied'), p('n_yielding'), float(w['v_floor']), float(w['brake']), int(w['detect']),
                                 int(w['n_per']), len(w['occupied']), len(w['conflict']), len(w['path_stop']), int(backwards))


copy_words = KH.copy_words


def blob(w, backwards):
    """a case of the stand-alone program's input file"""
    b = np.array([len(w['waited']), len(w['path_stop']), len(w['conflict']), w['n_per'], len(w['occupied']), w['detect'], int(w['done'] is not None),
                  int(backwards)], np.int32).tobytes()
    b += np.array([w['dl'], w['v_floor'], w['brake']], np.float64).tobytes() + w['state'].tobytes()
    for k in ('path_off', 'path_len', 'traj_idx', 'cut_len'):
        b += w[k].tobytes()
    if w['done'] is not None:
        b += w['done'].tobytes()
    for k in ('path_stop', 'path_move', 'path_exit', 'conflict', 'rank', 'gap', 'waited', 'yielding', 'blocker', 'lag', 'occupied', 'n_yielding'):
        b += w[k].tobytes()
    return b


def out_bytes(w, got):
    """what the stand-alone program writes for a case"""
    return b''.join(w[k].tobytes() for k in OUT_KEYS) + np.array([got], np.int32).tobytes()


def junctions(w, j0, j1):
    """the words of junctions [j0, j1) alone (the tables stay whole; blocker keeps the index of the whole batch)"""
    n = int(w['n_per'])
    out = dict(w)
    for k in PER_AGENT:
        out[k] = None if w[k] is None else w[k][j0 * n:j1 * n].copy()
    for k in PER_JUNCTION:
        out[k] = w[k][j0:j1].copy()
    return words(**out)


# ---------------------------------------------------------------- the hand-made junctions
# keepclear_helpers' four routes of 40 points in a table of 170: A = movement 0, line at local index 20, exit 30; B = movement 1 (A's lane),
# line 20, exit 30; Cc = movement 2, line 10, exit 25; D = movement 3, line 15, exit 28; points 160..169 defective.  Conflicts 0 - 2, 0 - 3,
# 1 - 2, 1 - 3, 2 - 3 (conflict = 12, 12, 11, 7): movements 0 and 1 share a lane and have no bit.  Ranks 2, 1, 0, 1: Cc is the major road, D
# and B come next, A is last.  Gaps 4, 0, 4, 3 seconds: movement 1 never gives way.  detect = 12 points, dl = 0.5 m, v_floor = 1 m/s,
# brake = 2 m/s^2: a car at v stops within v v / 4 metres.
A_, B_, C_, D_, DEF = KH.A_, KH.B_, KH.C_, KH.D_, KH.DEF
CONFLICT, RANK, GAP = (12, 12, 11, 7), (2, 1, 0, 1), (4.0, 0.0, 4.0, 3.0)
DETECT, DL, V_FLOOR, BRAKE = 12, 0.5, 1.0, 2.0
NAN = float('nan')
JUST_ABOVE_ONE = 1.0000000000000002     # the double behind 1.0
# an agent: (route, traj_idx, v, cut, waited, done)
PAD = (D_, 30, 0.0, 40, 0, 0)           # past its exit -- OUT (fills a junction)
C_IN = (C_, 12, 3.0, 40, 0, 0)          # movement 2 (rank 0) inside the crossing, behind its line (s = -1 there)
D_IN = (D_, 20, 3.0, 40, 0, 0)          # movement 3 (rank 1) inside
FREE = (0, 0, 40, -1, INF)              # want of an agent on a route of 40 points that the stage leaves alone
FREE10 = (0, 0, 10, -1, INF)

CASES = [
    # (what, agents) -> want (occupied, n_yielding, [(yielding, waited, cut, blocker as an index into the case's agents or -1, lag)])
    ('INSIDE of smaller rank: lag 0; it can stop, 5 points = 2.5 m >= 9 / 4', [C_IN, (A_, 15, 3.0, 40, 0, 0)], (4, 1, [FREE, (1, 1, 20, 0, 0.0)])),
    ('the same car in the next junction: the junction before does not leak', [(A_, 15, 3.0, 40, 1, 0)], (0, 0, [FREE])),
    ('INSIDE of equal rank (movements 1 and 3 conflict): no threat, a stale waited goes to 0', [(B_, 22, 3.0, 40, 0, 0), (D_, 10, 0.0, 40, 1, 0)], (2, 0, [FREE, FREE])),
    ('INSIDE of larger rank: no threat', [(A_, 22, 3.0, 40, 0, 0), (D_, 10, 0.0, 40, 1, 0)], (1, 0, [FREE, FREE])),
    ('no conflict bit (movement 1 inside, rank 1 < 2, the same lane): no threat', [(B_, 22, 3.0, 40, 0, 0), (A_, 15, 0.0, 40, 1, 0)], (2, 0, [FREE, FREE])),
    ('an APPROACH threat just below the gap: 8 points = 4 m at the double behind 1 m/s', [(C_, 2, JUST_ABOVE_ONE, 40, 0, 0), (A_, 15, 0.0, 40, 0, 0)],
     (0, 1, [FREE, (1, 1, 20, 0, 4.0 / JUST_ABOVE_ONE)])),
    ('exactly at the gap, 4 m at 1 m/s = 4 s: strict <, free, its lag and blocker are written', [(C_, 2, 1.0, 40, 0, 0), (A_, 15, 0.0, 40, 1, 0)],
     (0, 0, [FREE, (0, 0, 40, 0, 4.0)])),
    ('v below v_floor counts as v_floor: 4 points = 2 m at 0.25 m/s is 2 s, not 8, below D\'s gap of 3', [(C_, 6, 0.25, 40, 0, 0), (D_, 10, 0.0, 40, 0, 0)],
     (0, 1, [FREE, (1, 1, 15, 0, 2.0)])),
    ('a NaN speed counts as v_floor', [(C_, 6, NAN, 40, 0, 0), (D_, 10, 0.0, 40, 0, 0)], (0, 1, [FREE, (1, 1, 15, 0, 2.0)])),
    ('a candidate with a NaN speed cannot stop: free unless it waited', [C_IN, (A_, 15, NAN, 40, 0, 0), (D_, 10, NAN, 40, 1, 0)],
     (4, 1, [FREE, (0, 0, 40, 0, 0.0), (1, 1, 15, 0, 0.0)])),
    ('s - traj_idx = 12 = detect is looked at', [C_IN, (A_, 8, 0.0, 40, 0, 0)], (4, 1, [FREE, (1, 1, 20, 0, 0.0)])),
    ('beyond the detector (13 > 12): free, no lag, a stale waited goes to 0', [C_IN, (A_, 7, 0.0, 40, 1, 0)], (4, 0, [FREE, FREE])),
    ('a blocker beyond its own detector (15 > 12) still counts: 7.5 m at 2 m/s', [(D_, 0, 2.0, 40, 1, 0), (A_, 15, 0.0, 40, 0, 0)], (0, 1, [FREE, (1, 1, 20, 0, 3.75)])),
    ('a candidate that waited stays, whatever its speed', [C_IN, (A_, 15, 9.0, 40, 1, 0)], (4, 1, [FREE, (1, 1, 20, 0, 0.0)])),
    ('one that cannot stop: 2.5 m < 16 / 4 -- free, its lag is written', [C_IN, (A_, 15, 4.0, 40, 0, 0)], (4, 0, [FREE, (0, 0, 40, 0, 0.0)])),
    ('exactly on the stopping distance: 8 points = 4 m >= 16 / 4 holds', [C_IN, (A_, 12, 4.0, 40, 0, 0)], (4, 1, [FREE, (1, 1, 20, 0, 0.0)])),
    ('a tie of eta between two blockers, 2 m at 2 m/s each: the lowest index; the rank-1 blocker yields to the rank-0 one',
     [(A_, 15, 0.0, 40, 0, 0), (D_, 11, 2.0, 40, 0, 0), (C_, 6, 2.0, 40, 0, 0)], (0, 2, [(1, 1, 20, 1, 1.0), (1, 1, 15, 2, 1.0), FREE])),
    ('gap = 0: movement 1 never gives way, its lag is written', [C_IN, (B_, 15, 0.0, 40, 1, 0)], (4, 0, [FREE, (0, 0, 40, 0, 0.0)])),
    ('a conflict cut shorter than the line is kept', [C_IN, (A_, 15, 0.0, 17, 1, 0)], (4, 1, [FREE, (1, 1, 17, 0, 0.0)])),
    ('three ranks: rank 2 waits for the standing rank-1 car (0.5 m at v_floor), which waits for rank 0 (4 m at 2 m/s)',
     [(C_, 2, 2.0, 40, 0, 0), (D_, 14, 0.0, 40, 1, 0), (A_, 15, 0.0, 40, 1, 0)], (0, 2, [FREE, (1, 1, 15, 0, 2.0), (1, 1, 20, 1, 0.5)])),
    ('ON the line counts as INSIDE: rank 0 on its line blocks, and is never a candidate', [(C_, 10, 0.0, 40, 1, 0), (A_, 15, 0.0, 40, 1, 0)],
     (4, 1, [FREE, (1, 1, 20, 0, 0.0)])),
    ('one point before the exit still blocks', [(C_, 24, 3.0, 40, 0, 0), (A_, 19, 0.0, 40, 1, 0)], (4, 1, [FREE, (1, 1, 20, 0, 0.0)])),
    ('OUT: at its exit (ti == e) it blocks nobody', [(C_, 25, 3.0, 40, 0, 0), (A_, 19, 0.0, 40, 1, 0)], (0, 0, [FREE, FREE])),
    ('OUT: done inside the crossing (retired, or a slot at the gate)', [(C_, 12, 3.0, 40, 0, 1), (A_, 19, 0.0, 40, 1, 0)], (0, 0, [FREE, FREE])),
    ('OUT: a done candidate does not yield and its waited heals', [C_IN, (A_, 15, 0.0, 40, 1, 1)], (4, 0, [FREE, FREE])),
    ('OUT: movement 7 of 4', [C_IN, (DEF, 0, 0.0, 10, 1, 0)], (4, 0, [FREE, FREE10])),
    ('OUT: s = 12 >= path_len = 10', [C_IN, (DEF, 1, 0.0, 10, 1, 0)], (4, 0, [FREE, FREE10])),
    ('OUT: e = 11 > path_len = 10', [C_IN, (DEF, 2, 0.0, 10, 1, 0)], (4, 0, [FREE, FREE10])),
    ('OUT: a line ahead and e = -1', [C_IN, (DEF, 3, 0.0, 10, 1, 0)], (4, 0, [FREE, FREE10])),
    ('OUT: i = 173 outside [0, 170); i = -4', [C_IN, ((168, 10), 5, 0.0, 10, 1, 0), ((-9, 10), 5, 0.0, 10, 1, 0)], (4, 0, [FREE, FREE10, FREE10])),
    ('an empty junction', [], (0, 0, [])),
]

# junctions of 64 (n_per = 64 only): (what, slot -> agent) -> want (occupied, n_yielding, slot -> (yielding, waited, cut, blocker slot, lag))
WIDE = [
    ('63 waiting cars of movement 0 and one of movement 2 inside: 63 yield to it', lambda m: C_IN if m == 17 else (A_, 15, 0.0, 40, 1, 0),
     (4, 63, lambda m: FREE if m == 17 else (1, 1, 20, 17, 0.0))),
    ('movements 0 and 2 alternating in front of an empty box: the 32 of rank 2 yield to the first of rank 0, 2.5 m at v_floor',
     lambda m: (C_, 5, 0.0, 40, 1, 0) if m & 1 else (A_, 15, 0.0, 40, 1, 0), (0, 32, lambda m: FREE if m & 1 else (1, 1, 20, 1, 2.5))),
    ('the last lane alone inside (rank 1) beats the 32 approaching of rank 0 for the 31 of rank 2',
     lambda m: D_IN if m == 63 else (A_, 15, 0.0, 40, 1, 0) if m & 1 else (C_, 5, 0.0, 40, 1, 0),
     (8, 31, lambda m: FREE if m == 63 or not m & 1 else (1, 1, 20, 63, 0.0))),
]


def slots(n_agents, n_per):
    """where a case's agents sit in a junction of n_per: spread from the first slot to the last, in order"""
    return KH.slots(n_agents, n_per)


def _words_of(rows, J, n_per):
    stop, mv, ex = KH.tables()
    P = len(rows)
    col = lambda k: [r[k] for r in rows]
    state = np.zeros((P, 4)); state[:, 2] = col(2)
    return words(state=state, path_off=[r[0][0] for r in rows], path_len=[r[0][1] for r in rows], traj_idx=col(1), cut_len=col(3), waited=col(4),
                 done=col(5), yielding=np.full(P, -1), blocker=np.full(P, -7), lag=np.full(P, -1.0), path_stop=stop, path_move=mv, path_exit=ex,
                 conflict=CONFLICT, rank=RANK, gap=GAP, occupied=np.full(J, -1), n_yielding=np.full(J, -1), dl=DL, v_floor=V_FLOOR, brake=BRAKE,
                 detect=DETECT, n_per=n_per)


def hand_made(n_per, repeat=1):
    """CASES as junctions of n_per agents (the cases with more agents than n_per are left out), `repeat` times over, at n_per = 64 followed
    by WIDE; returns (words, want) with want = (occupied (J,), n_yielding (J,), {agent: (yielding, waited, cut, blocker, lag)}), blocker an
    agent index of the batch"""
    cases = [c for c in CASES if len(c[1]) <= n_per] * repeat
    rows, want_agent, head = [], {}, []
    for j, (_, agents, want) in enumerate(cases):
        rows += [PAD] * n_per
        sl = slots(len(agents), n_per)
        for slot, ag, wa in zip(sl, agents, want[2]):
            rows[j * n_per + slot] = ag
            want_agent[j * n_per + slot] = wa[:3] + (-1 if wa[3] < 0 else j * n_per + sl[wa[3]], wa[4])
        head.append(want[:2])
    if n_per == 64:
        for _, agent_at, want in WIDE:
            base = len(rows)
            rows += [agent_at(m) for m in range(64)]
            for m in range(64):
                wa = want[2](m)
                want_agent[base + m] = wa[:3] + (-1 if wa[3] < 0 else base + wa[3], wa[4])
            head.append(want[:2])
    w = _words_of(rows, len(head), n_per)
    return w, (np.array([h[0] for h in head], np.int32), np.array([h[1] for h in head], np.int32), want_agent)


def check_against_want(w, want, rows):
    """the words after the rule against the hand-written expectations; rows: the words before"""
    oc, ny, ag = want
    assert np.array_equal(w['occupied'], oc), np.flatnonzero(w['occupied'] != oc)
    assert np.array_equal(w['n_yielding'], ny), np.flatnonzero(w['n_yielding'] != ny)
    for q in range(len(w['yielding'])):
        exp = ag.get(q, (0, 0, int(rows['cut_len'][q]), -1, INF))         # (a padding agent is OUT)
        got = (int(w['yielding'][q]), int(w['waited'][q]), int(w['cut_len'][q]), int(w['blocker'][q]), float(w['lag'][q]))
        assert got[:4] == exp[:4] and np.float64(got[4]).tobytes() == np.float64(exp[4]).tobytes(), (q, got, exp)


def random_words(seed, n_per, J):
    """seeded random junctions on the tables of the hand-made ones: every route and the defective points, indices from before the route to
    behind its exit, speeds on both sides of v_floor and of the stopping distance (NaN among them), every waited word, retired agents,
    conflict cuts on both sides of the line; garbage in the out words"""
    rng = np.random.default_rng(seed)
    P = n_per * J
    routes = [A_, B_, C_, D_, DEF, (165, 10), (-3, 40)]
    pick = np.where(rng.random(P) < 0.7, rng.integers(0, 4, P), rng.integers(0, len(routes), P))
    rows = [(routes[k], int(rng.integers(-2, 34)), float(rng.choice([0.0, 0.25, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -4.0, NAN, rng.random() * 8])),
             int(rng.integers(5, 41)), int(rng.integers(0, 2)), int(rng.random() < 0.1)) for k in pick]
    w = _words_of(rows, J, n_per)
    w['yielding'] = rng.integers(-3, 4, P).astype(np.int32)
    w['blocker'] = rng.integers(-3, P + 3, P).astype(np.int32)
    w['lag'] = rng.random(P)
    return w


# ---------------------------------------------------------------- the oracle loop
ALWAYS_GREEN = dict(cycle=1, amber=0, green=np.array([[0, 1]] * 4))


def short_gap_entries(w, kinds, traj_before, drive):
    """the agents that make a SHORT-GAP ENTRY in a step: traj_idx passes the stop line (before < s <= after) while a conflicting car of
    smaller rank is inside the crossing or has eta < gap -- the rule's own lag of the step for the agent's movement, below its gap.  w: the
    rule's words of the step (traj_idx as the conflict search left it), kinds: their classification; returns [(agent, blocker, lag)]"""
    out = []
    agents = list(range(len(kinds)))
    for a in agents:
        if not drive[a]:
            continue
        i0 = int(w['path_off'][a]) + int(traj_before[a])
        s, m = int(w['path_stop'][i0]), int(w['path_move'][i0])
        if s >= 0 and traj_before[a] < s <= int(w['traj_idx'][a]) and kinds[a][0] != 'out':
            lag, blocker = meet(w, kinds, a, m, agents)
            if lag < np.float64(w['gap'][m]):
                out.append((a, blocker, float(lag)))
    return out


class PriorityLoop(G.SignalOracleLoop):
    """The step of an oracle loop of ONE junction without lights (SignalOracleLoop under a plan that is always green, for its clearance
    record and its clocks) under the priority rule, in the kernels' order: a conflict-search pass (the whole agent step of the oracle, whose
    solve stands for whoever is not cut) for all driving agents; the rule (rule_numpy) on the traj_idx those returned; then, for a yielding
    agent whose line lies below the returned cut (stop index), the window, rollout and QP again on full[:s] (speed mode: the whole path with
    the speed profile zeroed from s on) -- keepclear_helpers._KeepClearLoop.step with the rule in the hold's place.  move, exit: per agent,
    the route-local tables of its path; conflict, rank, gap: one word per movement; rule = False records what the rule would have seen
    and leaves the cars alone.  Records per step yielding, waited, blocker, lag, occ, the threatened candidates with their reason
    (candidates: (step, agent, movement, blocker, lag, why)) and the short-gap entries (entries: (step, agent, blocker, lag))."""

    def __init__(self, paths, dl, start, stop, group, move, exit, conflict, rank, gap, detect, v_floor=1.0, brake=None, rule=True, **kw):
        super().__init__(paths, dl, start, stop, group, ALWAYS_GREEN, brake=brake, **kw)
        offs = np.cumsum([0] + [len(p) for p in self.paths])
        gap = np.broadcast_to(np.asarray(gap, np.float64), (len(conflict),)).copy()
        self.tab = dict(path_stop=np.concatenate(self.stop), path_move=np.concatenate(move), path_exit=np.concatenate(exit), conflict=conflict,
                        rank=rank, gap=gap, dl=self.dl, v_floor=float(v_floor), brake=self.brake, detect=int(detect), n_per=self.A,
                        path_off=offs[:-1], path_len=[len(p) for p in self.paths])
        self.rule = bool(rule)
        self.movement = [int(np.asarray(m)[0]) for m in move]
        self.line = [int(np.asarray(s)[0]) for s in self.stop]
        A = self.A
        self.yielding, self.waited = np.zeros(A, np.int32), np.zeros(A, np.int32)
        self.blocker, self.lag = np.full(A, -1, np.int32), np.full(A, INF)
        self.occ_hist, self.candidates, self.entries = [], [], []
        self.yield_steps = np.zeros(A, np.int64)
        self.n_yielding = 0

    def step(self):
        from tests import speedref_helpers as S
        A, speed, p = self.A, self.speed, self.p
        pool = self.pool()
        self._measure(pool)
        gone = list(self.absent) + [False] * (len(pool) - A)
        res, present = [None] * A, [None] * A
        for a in range(A):
            if self.done[a]:
                continue
            present[a] = [r for r in range(len(pool)) if r != a and not gone[r]]
            step = S.agent_step if speed else orc.agent_step
            res[a] = step(p, np.ascontiguousarray(self.paths[a], np.float64), self.dl, self.state[a], pool[present[a]], self.traj_idx[a], self.prev[a],
                          self.target[a], self.u[a], self.centers, self.radius, self.margin)
        drive = [r is not None for r in res]
        ti = [int(res[a]['traj_idx']) if drive[a] else self.traj_idx[a] for a in range(A)]
        # the device's cut_len behind the conflict search: the cut length, in speed mode the stop index with the path length for "none"
        cut = [0] * A
        for a in range(A):
            if drive[a]:
                cut[a] = len(self.paths[a]) if res[a]['hit'] is None else int(res[a]['stop'] if speed else res[a]['cut'])
        w = words(state=self.state, traj_idx=ti, cut_len=cut, done=[0 if d else 1 for d in drive], waited=self.waited, yielding=self.yielding,
                  blocker=self.blocker, lag=self.lag, occupied=[0], n_yielding=[0], **self.tab)
        kinds = [KH.classify(w, q) for q in range(A)]
        self.entries += [(self.steps,) + e for e in short_gap_entries(w, kinds, self.traj_idx, drive)]
        log = []
        rule_numpy(w, log=log)
        self.occ_hist.append(int(w['occupied'][0]))
        if self.rule:
            self.yielding, self.waited, self.blocker, self.lag = w['yielding'], w['waited'], w['blocker'], w['lag']
            self.n_yielding = int(w['n_yielding'][0])
            self.candidates += [(self.steps, q, m, b, lag, why) for _, q, m, b, lag, why in log]
            cut = [int(v) for v in w['cut_len']]
            self.yield_steps += self.yielding != 0
        out = [None] * A
        new_state, new_applied = self.state.copy(), self.applied.copy()
        arrived = []
        for a in range(A):
            if not drive[a]:
                continue
            r, full, st = res[a], np.ascontiguousarray(self.paths[a], np.float64), self.state[a]
            sol, target = r['sol'], r['target_ind']
            before = len(full) if r['hit'] is None else int(r['stop'] if speed else r['cut'])
            if cut[a] < before:         # the re-solve of whoever the rule has cut, with the pieces agent_step itself calls
                uw = np.zeros((2, p.T)) if self.u[a] is None else np.asarray(self.u[a], float)
                if speed:
                    cv = S.speed_profile(len(full), cut[a])
                    xref, target, re = orc.calc_ref_trajectory(p, st, full[:, 0], full[:, 1], full[:, 2], self.dl, self.target[a], cv=cv)
                else:
                    tmp = full[:cut[a]]
                    xref, target, re = orc.calc_ref_trajectory(p, st, tmp[:, 0], tmp[:, 1], tmp[:, 2], self.dl, self.target[a])
                assert target >= 0
                xbar = orc.predict_motion(p, list(st), uw[0], uw[1])
                sol = orc.qp_solve(p, list(st), xref, xbar, re, uw)
            assert sol.status == 0, (self.steps, a, sol.status)
            length = len(full) if speed else cut[a]
            post = np.asarray(orc.plant_step(p, st, sol.u[0, 0], sol.u[1, 0]), dtype=np.float64)
            self.traj_idx[a], self.target[a], self.prev[a], self.u[a] = ti[a], int(target), int(length), sol.u.copy()
            new_state[a] = post
            new_applied[a] = (sol.u[1, 0], sol.u[0, 0])
            out[a] = dict(pool=pool, present=present[a], hit=-1 if r['hit'] is None else int(r['hit'][2]), cut=int(cut[a]), goal_len=int(length),
                          target=int(target), traj_idx=ti[a], x_sol=sol.x.copy(), u_sol=sol.u.copy(), post=post.copy(), ctrl=new_applied[a].copy(),
                          status=int(sol.status))
            if SH.is_goal(post, full[-1], target, length):
                arrived.append(a)
        self.state, self.applied = new_state, new_applied
        self.steps += 1
        for a in arrived:
            self.done[a], self.arrival[a] = True, self.steps
            self.applied[a] = 0.0
            if self.depart:
                self.absent[a] = True
        return out


# ---------------------------------------------------------------- the two scenes
# Stock routes (arm, turn), the major road being arms 1 and 3 (priority_ranks()' default).  TWO CARS: the straight from arm 1 (rank 0) from
# index 0 and the straight from arm 2 (rank 2) 60 points into its route.  FOUR CARS: the straight from arm 1, the turn across from arm 3
# (rank 1), the straights from arms 2 and 4 (rank 2).  gap 4 s, v_floor 1 m/s, brake = |MAX_DECEL|, detect = the whole approach, the full
# movement_conflicts() table, T = 13, v0 = 0, departure on.
SCENES = {'two': (((1, 2), (2, 2)), (0, 60)), 'four': (((1, 2), (3, 1), (2, 2), (4, 2)), (0, 0, 60, 30))}
SCENE_ROUTES = {'two': [[1, 3]], 'four': [[1, 4, 3, 7]]}       # the same as indices 2 (arm - 1) + (turn - 1) into stock_routes()' eight
GAP_S, V_FLOOR_S, STEPS = 4.0, 1.0, 250


def scene_tables(name):
    """(paths, dl, start, stop, group, move, exit, conflict, rank) of a scene: stop_lines()' and movement_lines()' rows per route,
    movement_conflicts() for the stock disc model, priority_ranks()"""
    from mpc_for_av_at_intersection_amd.batch import movement_conflicts, movement_lines, priority_ranks, stop_lines
    pairs, start = SCENES[name]
    paths = [H.smoothed_path(*pr) for pr in pairs]
    dl = float(np.linalg.norm(paths[0][0, :2] - paths[0][1, :2]))
    stop, group = stop_lines(paths)
    _, move, ex = movement_lines(paths)
    cd = SH.car()
    full, _ = movement_conflicts(paths, stop, ex, np.asarray(cd.circle_centers, dtype=np.float64), float(cd.radius))
    offs = np.cumsum([0] + [len(p) for p in paths])
    split = lambda t: [t[offs[k]:offs[k + 1]] for k in range(len(paths))]
    return paths, dl, list(start), split(stop), split(group), split(move), split(ex), full, priority_ranks()


def scene_loop(name, rule, speed=False, start=None, only=None):
    """a scene on the oracle; only: the agents kept (the others are left out: a solo run from the same start)"""
    paths, dl, st, stop, group, move, ex, conflict, rank = scene_tables(name)
    st = list(st if start is None else start)
    keep = list(range(len(paths))) if only is None else list(only)
    pick = lambda t: [t[k] for k in keep]
    detect = max(int(s[0]) for s in stop)
    return PriorityLoop(pick(paths), dl, pick(st), pick(stop), pick(group), pick(move), pick(ex), conflict, rank, GAP_S, detect, v_floor=V_FLOOR_S,
                        rule=rule, T=13, depart=True, speed=speed)


def ranks_of(loop):
    return [int(loop.tab['rank'][m]) for m in loop.movement]


# ---------------------------------------------------------------- the lifecycle
# One instance of eight slots with admission, respawn with routes, give_way('entry'), retirement with departure, following and the priority
# rule, cut mode: stack_helpers' scene 'plan' (instance 0: the first vehicles in line on the straight routes, the later ones from index 0)
# WITHOUT its lights.  Slots 0, 1, 4, 5 serve the major road (arms 1 and 3), slots 2, 3, 6, 7 the minor road.  flow_step is
# stack_helpers.stack_step's composition -- snapshot to snapshot, the order of enqueue_step -- with the priority rule in the hold's place,
# in front of the follower; it takes stack_helpers' own pieces for everything else (as keepclear_helpers.flow_step does).
FLOW_STEPS = 150
FLOW_INT = ('yielding', 'yield_waited', 'blocker', 'crossing', 'n_yielding')
FLOW_MINOR = (2, 3, 6, 7)


def flow_scene(routes):
    """(scene, tables): stack_helpers.scene('plan') cut to its first instance, and the per-path-point and per-movement tables of
    IntersectionBatch.priority_road()'s defaults"""
    from mpc_for_av_at_intersection_amd.batch import movement_conflicts, movement_lines, priority_ranks
    from tests import stack_helpers as K
    sc = K.scene('plan', routes)
    sc = dict(sc, route_of=sc['route_of'][:1], start_idx=sc['start_idx'][:1], due=sc['due'][:1])
    stop, move, ex = movement_lines(routes)
    cd = SH.car()
    full, _ = movement_conflicts(routes, stop, ex, np.asarray(cd.circle_centers, dtype=np.float64), float(cd.radius))
    return sc, dict(stop=stop, move=move, exit=ex, conflict=full, rank=priority_ranks(), gap=np.full(12, GAP_S), detect=int(stop.max()))


def flow_config(libs, routes, dl, rule=True):
    """(cfg, initial words) of the lifecycle scene for flow_step: stack_helpers.make_config with the rule's tables"""
    from tests import stack_helpers as K
    sc, tab = flow_scene(routes)
    cfg = K.make_config(libs, routes, dl, 1, K.A_, gap=sc['gap'], due=sc['due'], route_of=sc['route_of'], start_idx=sc['start_idx'], precedence='entry',
                        follow=sc['follow'])
    cfg.priority = None if not rule else dict(path_stop=tab['stop'], path_move=tab['move'], path_exit=tab['exit'], conflict=tab['conflict'],
                                              rank=tab['rank'], gap=tab['gap'], detect=tab['detect'], v_floor=V_FLOOR_S,
                                              brake=abs(float(cfg.p.max_decel)), dl=cfg.dl, n_per=cfg.A)
    w = K.initial_words(cfg, None, None)
    if rule:
        w.update(yielding=np.zeros(cfg.P, np.int32), yield_waited=np.zeros(cfg.P, np.int32), blocker=np.full(cfg.P, -1, np.int32), lag=np.full(cfg.P, INF),
                 crossing=np.zeros(1, np.int32), n_yielding=np.zeros(1, np.int32))
    return cfg, w


def flow_step(cfg, before):
    """One step of the lifecycle scene: the words after it from the words before it (neither is modified) and what happened in it,
    (after, info) with info = dict(agents={q: ...}, admitted, arrived, candidates=[(junction, agent, movement, blocker, lag, why)],
    entries=[(agent, blocker, lag)])"""
    from tests import follow_helpers as FH
    from tests import intent_helpers as IH
    from tests import precedence_helpers as PR
    from tests import stack_helpers as K
    P, p = cfg.P, cfg.p
    w = {k: np.array(v, copy=True) for k, v in before.items()}
    own = cfg.obs_skip
    done0 = before['done'].copy()
    K._admit(cfg, w)
    admitted = [q for q in range(P) if done0[q] and not w['done'][q]]
    PR.host_stamp(cfg.libs.stamp, w['precedence'], w['entered_step'], own, cfg.obs_off, P)
    done, absent = w['done'].copy(), w['absent'].copy()
    pool = np.column_stack([before['state'], before['applied'][:, 1], before['applied'][:, 0]])
    drive = [q for q in range(P) if not done[q]]
    cache = {}

    def seen(r, stand):
        if (r, stand) not in cache:
            cache[r, stand] = (orc.predict_obstacle(PR.standing(pool[r:r + 1], [0])[0], p.dt, p.L, cfg.pred_steps) if stand else
                               orc.predict_obstacle(pool[r], p.dt, p.L, cfg.pred_steps))
        return cache[r, stand]
    agents = {}
    for q in drive:         # the conflict search
        full = cfg.path[before['path_off'][q]:before['path_off'][q] + before['path_len'][q]]
        present = [r for r in range(cfg.obs_off[q], cfg.obs_off[q] + cfg.obs_cnt[q]) if r != own[q] and not absent[r]]
        trajs = [seen(r, bool(w['precedence'][r] > w['precedence'][own[q]])) for r in present]
        ti, hit, cut, _ = IH.intent_search(p, full, before['state'][q], trajs, int(before['traj_idx'][q]), int(before['cut_len'][q]), cfg.centers,
                                           cfg.radius, cfg.margin, False, cfg.frame_window, cfg.max_accel)
        if hit is None:
            cut = len(full)
        agents[q] = dict(full=full, conflict_cut=int(cut))
        w['traj_idx'][q], w['cut_len'][q], w['hit_idx'][q] = ti, cut, -1 if hit is None else int(hit[2])
    # the priority rule, in the hold's place
    log, entries = [], []
    if cfg.priority is not None:
        kw = words(state=before['state'], path_off=before['path_off'], path_len=before['path_len'], traj_idx=w['traj_idx'], cut_len=w['cut_len'],
                   done=done, waited=w['yield_waited'], yielding=w['yielding'], blocker=w['blocker'], lag=w['lag'], occupied=w['crossing'],
                   n_yielding=w['n_yielding'], **cfg.priority)
        kinds = [KH.classify(kw, q) for q in range(P)]
        entries = short_gap_entries(kw, kinds, before['traj_idx'], [not d for d in done])
        rule_numpy(kw, log=log)
        w.update(cut_len=kw['cut_len'], yielding=kw['yielding'], yield_waited=kw['waited'], blocker=kw['blocker'], lag=kw['lag'],
                 crossing=kw['occupied'], n_yielding=kw['n_yielding'])
    # following and the solve
    w['leader'][:], w['gap'][:], w['follow_cap'][:] = -1, -1.0, 0.0
    for q in drive:
        a = agents[q]
        full, ti, st = a['full'], int(w['traj_idx'][q]), before['state'][q]
        cut = int(w['cut_len'][q])
        slots_ = FH.others_of(int(cfg.obs_off[q]), int(cfg.obs_cnt[q]), int(own[q]), P, absent)
        best = FH.leader_of(full, ti, pool, slots_, cfg.follow, cfg.follow['reach'])
        if best is not None:
            gap, s, cap = FH.stop_and_cap(ti, best[1], best[2], st[2], cfg.dl, False, cfg.follow)
            w['leader'][q], w['gap'][q], w['follow_cap'][q] = best[0], gap, cap
            cut = min(cut, s)
        r = IH.intent_solve(p, full, cfg.dl, st, int(before['target_ind'][q]), before['u'][q], cut, False)
        sol = r['sol']
        assert sol.status == 0, (q, sol.status)
        w['cut_len'][q], w['target_ind'][q], w['status'][q], w['iters'][q] = cut, r['target_ind'], sol.status, sol.iters
        w['u'][q], w['x'][q], w['xref'][q] = sol.u, sol.x, r['xref']
        w['state'][q] = orc.plant_step(p, st, sol.u[0, 0], sol.u[1, 0])
        w['applied'][q] = (sol.u[1, 0], sol.u[0, 0])
        a.update(cut=cut)
    K._retire(cfg, w)
    arrived = [q for q in drive if w['done'][q]]
    K._respawn(cfg, w)
    return w, dict(agents=agents, admitted=admitted, arrived=arrived, candidates=log, entries=entries, pool=pool)
