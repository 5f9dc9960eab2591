"""Traffic signals (mpcx_signals: an agent whose light is red -- or amber, if it can stop -- is held at its stop line) for the tests: the
closed loop of several egos on the CPU oracle under the rule (SignalOracleLoop, a subclass of scene_helpers.OracleLoop), a numpy restatement
of the rule, the host build of csrc/mpcx_signal_core.h (tests/signal_ref/signal_ref.cpp) behind numpy arrays, the hand-made words of
tests/test_signal_cpu.py and the scene both test files run: four straight stock routes from index 0 under a two-phase plan.

The rule shortens the cut length (the stop index in speed mode) the conflict search produced to the agent's stop line s, and nothing else:
a step with signals is the step without them with min(cut, s) in place of cut for every held agent."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle_py as orc
from tests import helpers as H
from tests import scene_helpers as SH

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'signal_ref', 'signal_ref.cpp')
INC = ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc')]
GREEN, AMBER, RED = 0, 1, 2
HALF_WIDTH = 12.0       # the stock crossing: a square of this half width about the origin

# the plan tests/test_signal_cpu.py picks on the oracle run of the straight scene, and what that run gives (S3)
PLAN = dict(cycle=100, green=30, amber=8)        # the all-red gap that follows: 50 - 30 - 8 = 12 steps


def light(cycle, amber, green_from, green_len, t):
    u = t - green_from
    if u < 0:
        u += cycle
    return GREEN if u < green_len else AMBER if u < green_len + amber else RED


def rule_numpy(w):
    """the rule restated on a dict of numpy arrays (state, path_off, path_len, traj_idx, cut_len, done or None, path_stop, path_group,
    plan_cycle, plan_amber, plan_green (n_plans, n_groups, 2), plan_of, tick, held, dl, brake), in place on cut_len, tick and held; returns
    the number of agents held"""
    n_points, (n_plans, n_groups, _) = len(w['path_stop']), w['plan_green'].shape
    got = 0
    for q in range(len(w['plan_of'])):
        plan = int(w['plan_of'][q])
        cycle = int(w['plan_cycle'][plan]) if 0 <= plan < n_plans else 0
        t = 0
        if cycle >= 1:
            t = int(w['tick'][q]) % cycle            # (Python's % is already non-negative)
            w['tick'][q] = (t + 1) % cycle
        if w.get('done') is not None and w['done'][q]:
            w['held'][q] = 0
            continue
        ti = int(w['traj_idx'][q])
        i = int(w['path_off'][q]) + ti
        held = 0
        if cycle >= 1 and 0 <= i < n_points:
            s, g = int(w['path_stop'][i]), int(w['path_group'][i])
            if 0 <= s < int(w['path_len'][q]) and ti < s and 0 <= g < n_groups:
                lt = light(cycle, int(w['plan_amber'][plan]), int(w['plan_green'][plan, g, 0]), int(w['plan_green'][plan, g, 1]), t)
                if lt == RED:
                    held = 1
                elif lt == AMBER:
                    v = np.float64(w['state'][q, 2])
                    if w['held'][q] != 0 or np.float64(s - ti) * np.float64(w['dl']) >= v * v / (np.float64(2.0) * np.float64(w['brake'])):
                        held = 2
                if held and s < w['cut_len'][q]:
                    w['cut_len'][q] = s
        w['held'][q] = held
        got += held != 0
    return got


def build_ref(directory):
    """the host build of the rule as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    so = os.path.join(str(directory), 'libsignal_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.signal_ref_step.restype = C.c_int
    lib.signal_ref_step.argtypes = [C.c_int, C.c_double] + [C.c_void_p] * 14 + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.signal_ref_layout.restype = None
    return lib


I32_KEYS = ('path_off', 'path_len', 'traj_idx', 'cut_len', 'path_stop', 'path_group', 'plan_cycle', 'plan_amber', 'plan_green', 'plan_of', 'tick',
            'held')


def words(**kw):
    """a dict of the rule's words with the dtypes and layouts the host build takes"""
    w = dict(kw)
    for k in I32_KEYS:
        w[k] = np.ascontiguousarray(w[k], dtype=np.int32)
    w['state'] = np.ascontiguousarray(w['state'], dtype=np.float64)
    w['done'] = None if w.get('done') is None else np.ascontiguousarray(w['done'], dtype=np.int32)
    return w


def host_rule(lib, w, backwards=False):
    """the rule through the host build, in place on w['cut_len'], w['tick'], w['held'] (a dict from words()); returns the number held"""
    p = lambda k: None if w[k] is None else w[k].ctypes.data
    n_plans, n_groups, _ = w['plan_green'].shape
    return lib.signal_ref_step(len(w['plan_of']), float(w['dl']), p('state'), p('path_off'), p('path_len'), p('traj_idx'), p('cut_len'), p('done'),
                               p('path_stop'), p('path_group'), p('plan_cycle'), p('plan_amber'), p('plan_green'), p('plan_of'), p('tick'),
                               p('held'), float(w['brake']), len(w['path_stop']), n_plans, n_groups, int(backwards))


def copy_words(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def hand_made():
    """Hand-made words: two routes in a table of 50 points -- route A = points 0..29 with its line at local index 20 (group 0), route B =
    points 30..49 with its line at local index 10 (group 1) and nothing behind it.  Two plans over two groups: plan 0 has cycle 10, amber
    2, group 0 green from 0 for 4 (amber at t = 4, 5; red from 6), group 1 green from 5 for 3 (amber 8, 9; red 0..4); plan 1 has cycle 7,
    amber 0, both groups green from 3 for 4 (red 0..2).  dl = 0.5, brake = 2: a car at v stops within v v / 4 metres.
    What each agent is there for, and what the rule must make of it (held, cut_len, tick), stands beside its row below; returns (words, want)."""
    stop = np.full(50, -1, np.int32); grp = np.zeros(50, np.int32)
    stop[0:21] = 20; stop[30:41] = 10; grp[30:41] = 1
    grp[45] = 7; stop[45] = 18            # a defective point: a group that does not exist (agent 12 stands on it)
    stop[46] = 25                         # a defective point: a line beyond the route's end (agent 13)
    stop[22] = 20                         # a table that still names the line behind the point: past the line (agent 0)
    A, B = (0, 30), (30, 20)
    rows = [
        # (route, traj_idx, v, cut, plan, tick, held, done) -> want (held, cut, tick)
        (A, 22, 3.0, 30, 0, 7, 0, 0, (0, 30, 8)),     # 0  past the line at red
        (A, 20, 3.0, 30, 0, 7, 1, 0, (0, 30, 8)),     # 1  ON the line at red: free, and a previous hold is dropped
        (B, 12, 1.0, 20, 0, 0, 0, 0, (0, 20, 1)),     # 2  no line ahead (s = -1)
        (A, 5, 3.0, 30, 0, 2, 0, 0, (0, 30, 3)),      # 3  GREEN
        (A, 5, 3.0, 30, 0, 6, 0, 0, (1, 20, 7)),      # 4  RED: cut 30 -> 20
        (A, 5, 3.0, 12, 0, 6, 0, 0, (1, 12, 7)),      # 5  RED with a conflict cut shorter than s: kept
        (A, 10, 4.0, 30, 0, 4, 0, 0, (2, 20, 5)),     # 6  AMBER, can stop: (20 - 10) 0.5 = 5 >= 16 / 4 = 4
        (A, 10, 5.0, 30, 0, 5, 0, 0, (0, 30, 6)),     # 7  AMBER, cannot stop: 5 < 25 / 4
        (A, 10, 5.0, 30, 0, 5, 2, 0, (2, 20, 6)),     # 8  AMBER, cannot stop but held before: sticky
        (A, 5, 3.0, 30, 0, 6, 1, 1, (0, 30, 7)),      # 9  retired at red: held cleared, cut untouched, the clock still runs
        (A, 5, 3.0, 30, 0, 9, 0, 0, (1, 20, 0)),      # 10 tick wraps at cycle - 1
        (A, 5, 3.0, 30, 0, -3, 0, 0, (1, 20, 8)),     # 11 negative tick: -3 -> 7 (red) -> 8
        (B, 15, 1.0, 20, 0, 0, 0, 0, (0, 20, 1)),     # 12 defective: group 7 of 2
        (B, 16, 1.0, 20, 0, 0, 0, 0, (0, 20, 1)),     # 13 defective: s = 25 >= path_len = 20
        (A, 5, 3.0, 30, 2, 6, 1, 0, (0, 30, 6)),      # 14 defective: plan 2 of 2 -- no cycle, the tick stays
        (A, 5, 3.0, 30, -1, 6, 0, 0, (0, 30, 6)),     # 15 defective: plan -1
        ((40, 30), 5, 3.0, 30, 0, 6, 0, 0, (0, 30, 7)),   # 16 defective: path_off + traj_idx = 45 ... its route runs past the table; point 45 has group 7
        ((48, 30), 5, 3.0, 30, 0, 6, 0, 0, (0, 30, 7)),   # 17 defective: i = 53 outside [0, 50)
        ((-9, 30), 5, 3.0, 30, 0, 6, 0, 0, (0, 30, 7)),   # 18 defective: i = -4
        (B, 3, 1.0, 20, 0, 25, 0, 0, (0, 20, 6)),     # 19 over-range tick 25 -> 5: group 1 GREEN from 5
        (B, 3, 1.0, 20, 1, 1, 0, 0, (1, 10, 2)),      # 20 plan 1 (cycle 7): red at 1
        (B, 3, 1.0, 20, 1, 6, 0, 0, (0, 20, 0)),      # 21 plan 1: green at 6, wraps to 0
    ]
    P = len(rows)
    state = np.zeros((P, 4)); state[:, 2] = [r[2] for r in rows]
    w = words(state=state, path_off=[r[0][0] for r in rows], path_len=[r[0][1] for r in rows], traj_idx=[r[1] for r in rows],
              cut_len=[r[3] for r in rows], done=[r[7] for r in rows], path_stop=stop, path_group=grp, plan_cycle=[10, 7], plan_amber=[2, 0],
              plan_green=np.array([[[0, 4], [5, 3]], [[3, 4], [3, 4]]]), plan_of=[r[4] for r in rows], tick=[r[5] for r in rows],
              held=[r[6] for r in rows], dl=0.5, brake=2.0)
    want = np.array([r[8] for r in rows], np.int32)
    return w, want


def blob(w, backwards):
    """a case of the stand-alone program's input file"""
    n_plans, n_groups, _ = w['plan_green'].shape
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    b = i32(len(w['plan_of']), len(w['path_stop']), n_plans, n_groups, int(w['done'] is not None), int(backwards))
    b += np.array([w['dl'], w['brake']], np.float64).tobytes() + w['state'].tobytes()
    for k in ('path_off', 'path_len', 'traj_idx', 'cut_len'):
        b += w[k].tobytes()
    if w['done'] is not None:
        b += w['done'].tobytes()
    for k in ('path_stop', 'path_group', 'plan_cycle', 'plan_amber', 'plan_green', 'plan_of', 'tick', 'held'):
        b += w[k].tobytes()
    return b


# ---------------------------------------------------------------- the oracle step
def signal_agent_step(p, full, dl, st, rows, traj_idx, prev, target, u, centers, radius, margin, speed, decide, v_ref=None):
    """One agent's step under the rule: orc.agent_step (speedref_helpers.agent_step in speed mode), then decide(traj_idx, v) -> (held, s)
    on the traj_idx the step returned, and, for a held agent whose line s lies below the returned cut (stop index), only the window, rollout
    and QP again on full[:s] (speed mode: the whole path with the speed profile zeroed from s on), with the pieces agent_step itself calls.
    Returns agent_step's dict with `cut` (speed mode: the stop index, 999 = none), `held`, `line` and the sol / target_ind that hold."""
    from tests import speedref_helpers as S
    full = np.ascontiguousarray(full, np.float64)
    kw = {} if v_ref is None else dict(v_ref=v_ref)
    if speed:
        r = S.agent_step(p, full, dl, st, rows, traj_idx, prev, target, u, centers, radius, margin, **kw)
        cut = r['stop']
    else:
        r = orc.agent_step(p, full, dl, st, rows, traj_idx, prev, target, u, centers, radius, margin)
        cut = r['cut']
    held, s = decide(int(r['traj_idx']), st[2])
    r = dict(r, held=int(held), line=int(s))
    if held and s < cut:
        cut = s
        uw = np.zeros((2, p.T)) if u is None else np.asarray(u, float)
        if speed:
            cv = S.speed_profile(len(full), s, **kw)
            xref, tgt, re = orc.calc_ref_trajectory(p, st, full[:, 0], full[:, 1], full[:, 2], dl, target, cv=cv)
        else:
            tmp = full[:s]
            xref, tgt, re = orc.calc_ref_trajectory(p, st, tmp[:, 0], tmp[:, 1], tmp[:, 2], dl, target)
        assert tgt >= 0
        xbar = orc.predict_motion(p, list(st), uw[0], uw[1])
        r.update(target_ind=tgt, xref=xref, xbar=xbar, re=re, sol=orc.qp_solve(p, list(st), xref, xbar, re, uw))
    r['cut'] = int(cut)
    return r


# ---------------------------------------------------------------- the oracle loop
class SignalOracleLoop(SH.OracleLoop):
    """OracleLoop with the signal rule.  stop, group: per agent, the route-local tables of its path (stop_lines()' rows of its route);
    plan: dict(cycle, amber, green (n_groups, 2)); tick: the agents' initial clocks (default 0).  Per agent: orc.agent_step (or the speed
    mode's), then, for a held agent whose line s lies below the returned cut, only the window, rollout and QP again on full[:s] (speed mode:
    on the whole path with the speed profile zeroed from s), with the pieces agent_step itself calls; prev_cut = s is carried.  Records
    held per step, the true clearance between the present, driving agents at the start of every step and the steps in which agents of
    different groups were inside the crossing square together."""

    def __init__(self, paths, dl, start, stop, group, plan, tick=None, brake=None, **kw):
        super().__init__(paths, dl, start, **kw)
        self.stop, self.group, self.plan = stop, group, plan
        self.tick = [0] * self.A if tick is None else [int(t) for t in tick]
        self.held = [0] * self.A
        self.brake = abs(float(self.p.max_decel)) if brake is None else float(brake)
        self.worst_clearance = np.inf
        self.amber_free = 0
        self.mixed_steps = []               # steps at whose start cars of different groups were inside the square together
        self.phase_of = [tuple(int(v) for v in plan['green'][int(np.asarray(g)[0])]) for g in group]      # equal greens = one phase

    def _measure(self, pool):
        live = [a for a in range(self.A) if not self.done[a] and not self.absent[a]]
        for a in live:
            others = [r for r in live if r != a]
            if others:
                self.worst_clearance = min(self.worst_clearance, SH.clearance(pool, a, others, self.centers, self.radius))
        inside = {self.phase_of[a] for a in live if max(abs(pool[a, 0]), abs(pool[a, 1])) <= HALF_WIDTH}
        if len(inside) > 1:
            self.mixed_steps.append(self.steps)

    def _decide(self, a, ti, v):
        """steps 3 and 4 of the rule for a driving agent; returns (held, s)"""
        pl = self.plan
        t = self.tick[a] % pl['cycle']
        s, g = int(self.stop[a][ti]), int(self.group[a][ti])
        if s < 0 or ti >= s or s >= len(self.paths[a]) or not 0 <= g < len(pl['green']):
            return 0, s
        lt = light(pl['cycle'], pl['amber'], int(pl['green'][g][0]), int(pl['green'][g][1]), t)
        if lt == RED:
            return 1, s
        if lt == AMBER and (self.held[a] != 0 or np.float64(s - ti) * np.float64(self.dl) >= np.float64(v) * np.float64(v) / (2.0 * self.brake)):
            return 2, s
        self.amber_free += lt == AMBER      # in front of its line in amber and not held: it cannot stop
        return 0, s

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
            r = signal_agent_step(self.p, full, self.dl, st, pool[present], self.traj_idx[a], self.prev[a], self.target[a], self.u[a], self.centers,
                                  self.radius, self.margin, self.speed, lambda ti, v, a=a: self._decide(a, ti, v))
            held, cut, sol, target = r['held'], r['cut'], r['sol'], r['target_ind']
            self.held[a] = held
            length = len(full) if self.speed else cut
            assert sol.status == 0, (self.steps, a, sol.status)
            post = np.asarray(orc.plant_step(self.p, st, sol.u[0, 0], sol.u[1, 0]), dtype=np.float64)
            self.traj_idx[a], self.target[a], self.prev[a], self.u[a] = int(r['traj_idx']), int(target), int(length), sol.u.copy()
            new_state[a] = post
            new_applied[a] = (sol.u[1, 0], sol.u[0, 0])
            out[a] = dict(pool=pool, present=present, hit=-1 if r['hit'] is None else int(r['hit'][2]), cut=int(cut), goal_len=int(length),
                          target=int(target), traj_idx=int(r['traj_idx']), x_sol=sol.x.copy(), u_sol=sol.u.copy(), post=post.copy(),
                          ctrl=new_applied[a].copy(), status=int(sol.status), held=int(held))
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


def straight_scene():
    """(paths, dl, start, stop, group): the four straight stock routes from index 0 with their stop lines"""
    from mpc_for_av_at_intersection_amd.batch import stop_lines
    paths = [H.smoothed_path(a, 2) for a in (1, 2, 3, 4)]
    dl = float(np.linalg.norm(paths[0][0, :2] - paths[0][1, :2]))
    stop, group = stop_lines(paths)
    offs = np.cumsum([0] + [len(p) for p in paths])
    split = lambda t: [t[offs[k]:offs[k + 1]] for k in range(len(paths))]
    return paths, dl, [0] * 4, split(stop), split(group)


def straight_loop(plan=None, tick=None, speed=False):
    from mpc_for_av_at_intersection_amd.batch import two_phase_plan
    paths, dl, start, stop, group = straight_scene()
    if plan is None:
        plan = two_phase_plan(**PLAN)
    return SignalOracleLoop(paths, dl, start, stop, group, plan, tick=tick, T=13, depart=True, speed=speed)
