"""Respawn (mpcx_respawn: a departed agent's slot is re-used for the next vehicle) for the tests: the host build of
csrc/mpcx_respawn_core.h (tests/respawn_ref/respawn_ref.cpp) behind numpy arrays, a numpy restatement of the rule, the hand-made words that
tests/test_respawn_cpu.py runs through the host build and tests/test_gpu_respawn.py through the device stage, and the closed loop of several
egos on the CPU oracle with admission at the head and respawn at the end of every step (RespawnOracleLoop)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import admit_helpers as AH

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'respawn_ref', 'respawn_ref.cpp')
INC = AH.INC
# the words the rule may write, in the order respawn_ref.cpp's main() writes them back
MUT_F64 = ('state', 'applied', 'u', 'ep_f64', 'min_clearance')
MUT_I32 = ('traj_idx', 'target_ind', 'cut_len', 'iters', 'prev_len', 'steps_driven', 'wait', 'entered', 'served', 'ep_i32', 'lsteps', 'goal_step',
           'contact_step', 'flags')
CONST_I32 = ('own', 'done', 'clock', 'start_idx', 'due')


def build_ref(directory):
    """the host build as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    from mpc_for_av_at_intersection_amd import _lib
    so = os.path.join(str(directory), 'librespawn_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.respawn_ref_step.restype = C.c_int
    lib.respawn_ref_step.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 9 + [C.POINTER(_lib.RunLogC), C.POINTER(_lib.RetireC), C.POINTER(_lib.AdmitC),
                                                                       C.POINTER(_lib.RespawnC), C.c_int])
    lib.respawn_ref_layout.restype = None
    return lib


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class Case:
    """the words of P agents that the rule reads and writes, as numpy arrays.  log / speed: whether the run has a log / a prev_len (the
    arrays exist all the same and must then stay untouched)"""

    def __init__(self, P, T, G, n_pool, log=True, speed=False, **words):
        self.P, self.T, self.G, self.n_pool, self.log, self.speed = int(P), int(T), int(G), int(n_pool), bool(log), bool(speed)
        shapes = dict(state=(P, 4), applied=(P, 2), u=(P, 2 * T), ep_f64=(P, G, 2), min_clearance=(P,), start_state=(P, 4))
        for k in MUT_F64 + ('start_state',):
            setattr(self, k, _f64(words[k] if k in words else np.zeros(shapes[k])).reshape(shapes[k]).copy())
        ishapes = dict(ep_i32=(P, G, 8), due=(P, G), clock=(1,))
        for k in MUT_I32 + CONST_I32:
            shape = ishapes.get(k, (P,))
            setattr(self, k, _i32(words[k] if k in words else np.zeros(shape)).reshape(shape).copy())

    def copy(self):
        return Case(self.P, self.T, self.G, self.n_pool, self.log, self.speed,
                    **{k: getattr(self, k) for k in MUT_F64 + MUT_I32 + CONST_I32 + ('start_state',)})

    def words(self):
        return {k: getattr(self, k).copy() for k in MUT_F64 + MUT_I32}

    def blob(self):
        """the mutable words as respawn_ref.cpp's main() writes them back (without the count of arrivals)"""
        return b''.join(getattr(self, k).tobytes() for k in MUT_F64 + MUT_I32)

    def serialise(self, backwards, steps):
        """the record tests/respawn_ref/respawn_ref.cpp's main() reads"""
        head = np.array([self.P, self.n_pool, 2 * self.T, self.G, int(self.log), int(self.speed), int(backwards), steps], np.int32)
        order = ('state', 'applied', 'u', 'start_state', 'ep_f64', 'min_clearance', 'traj_idx', 'target_ind', 'cut_len', 'iters', 'prev_len', 'own', 'done',
                 'steps_driven', 'wait', 'entered', 'clock', 'start_idx', 'due', 'served', 'ep_i32', 'lsteps', 'goal_step', 'contact_step', 'flags')
        return head.tobytes() + b''.join(getattr(self, k).tobytes() for k in order)


def structs(case, ptr=lambda a: a.ctypes.data):
    """(RunLogC or None, RetireC, AdmitC, RespawnC) naming the arrays of `case` (ptr: array -> address)"""
    from mpc_for_av_at_intersection_amd import _lib
    log = None
    if case.log:
        log = _lib.RunLogC()
        log.capacity, log.goal_dis, log.stop_speed = 0, 1.5, 0.1389
        log.steps, log.goal_step, log.contact_step, log.flags, log.min_clearance = (ptr(getattr(case, k)) for k in
                                                                                      ('lsteps', 'goal_step', 'contact_step', 'flags', 'min_clearance'))
    retire = _lib.RetireC(ptr(case.done), ptr(case.steps_driven), 1.5, 0.1389)
    admit = _lib.AdmitC(ptr(case.wait), ptr(case.entered), ptr(case.clock), 0, 0.0)
    rs = _lib.RespawnC(case.G, 0, ptr(case.start_state), ptr(case.start_idx), ptr(case.due), ptr(case.served), ptr(case.ep_i32), ptr(case.ep_f64))
    return log, retire, admit, rs


def host_step(lib, case, backwards=False):
    """one step of the rule on `case`, in place, through the host build; returns the number of agents that arrived"""
    log, retire, admit, rs = structs(case)
    return lib.respawn_ref_step(case.P, case.n_pool, 2 * case.T, case.state.ctypes.data, case.applied.ctypes.data, case.u.ctypes.data,
                                case.traj_idx.ctypes.data, case.target_ind.ctypes.data, case.cut_len.ctypes.data, case.iters.ctypes.data,
                                case.prev_len.ctypes.data if case.speed else None, case.own.ctypes.data,
                                None if log is None else C.byref(log), C.byref(retire), C.byref(admit), C.byref(rs), int(backwards))


def numpy_step(c):
    """The rule restated in numpy, in place on `c`; returns the list of agents that arrived."""
    clock = int(c.clock[0])
    arrived = [q for q in range(c.P) if c.done[q] != 0 and c.wait[q] == -1 and c.entered[q] >= 0 and c.served[q] < c.G and 0 <= c.own[q] < c.n_pool]
    for q in arrived:
        g = int(c.served[q])
        c.ep_i32[q, g] = [c.entered[q], clock - 1, c.steps_driven[q], c.lsteps[q] if c.log else -1, c.contact_step[q] if c.log else -1,
                          c.flags[q] if c.log else 0, c.due[q, g], 0]
        c.ep_f64[q, g] = [c.min_clearance[q] if c.log else np.inf, 0.0]
        c.served[q] = g + 1
        if g + 1 == c.G:
            continue
        c.state[q], c.applied[q], c.u[q] = c.start_state[q], 0.0, 0.0
        c.traj_idx[q] = c.target_ind[q] = c.start_idx[q]
        c.cut_len[q] = c.iters[q] = c.steps_driven[q] = 0
        if c.speed:
            c.prev_len[q] = 0
        if c.log:
            c.goal_step[q] = c.contact_step[q] = -1
            c.flags[q], c.min_clearance[q] = 0, np.inf
        c.entered[q] = -1
        c.wait[q] = max(0, int(c.due[q, g + 1]) - clock)
    return arrived


# ---------------------------------------------------------------- the hand-made words
BRANCHES = ('driving', 'waiting', 'future due', 'past due', 'last vehicle', 'finished', 'own row outside', 'due now', 'never entered')


def hand_made(log=True, speed=False, seed=7):
    """Nine agents, one per branch (BRANCHES), T = 3, G = 3, a pool of nine rows, the clock at 20 (this step is step 19):
       0 driving; 1 waiting (wait 4); 2 arrived, one vehicle served before... none: served 0, its next vehicle due at step 50 -> wait 30;
       3 arrived, served 1, next due at step 7 (past) -> wait 0; 4 arrived with served 2: the last vehicle, record and no reset;
       5 served == G: untouched; 6 arrived but its own row (11) lies outside the pool: untouched; 7 due (wait 0, not yet in): untouched;
       8 retired and never entered (entered_step -1, wait -1: a hidden agent): untouched.
    Every word that a reset writes holds something else before."""
    rng = np.random.default_rng(seed)
    P, T, G = 9, 3, 3
    w = dict(state=rng.normal(size=(P, 4)), applied=rng.normal(size=(P, 2)), u=rng.normal(size=(P, 2 * T)), start_state=rng.normal(size=(P, 4)),
             ep_f64=np.full((P, G, 2), -7.0), min_clearance=rng.uniform(0.1, 3.0, P),
             traj_idx=rng.integers(100, 200, P), target_ind=rng.integers(100, 200, P), cut_len=rng.integers(200, 300, P), iters=rng.integers(3, 9, P),
             prev_len=rng.integers(300, 400, P), steps_driven=rng.integers(10, 19, P), lsteps=rng.integers(40, 60, P), goal_step=rng.integers(40, 60, P),
             contact_step=[-1, -1, 41, -1, -1, -1, -1, -1, -1], flags=[1, 0, 1, 1, 0, 1, 1, 0, 0], start_idx=rng.integers(0, 50, P),
             ep_i32=np.full((P, G, 8), -7), own=[0, 1, 2, 3, 4, 5, 11, 7, 8], done=[0, 1, 1, 1, 1, 1, 1, 1, 1],
             wait=[-1, 4, -1, -1, -1, -1, -1, 0, -1], entered=[2, -1, 5, 3, 8, 9, 4, -1, -1], clock=[20],
             due=[[0, 1, 2], [4, 30, 31], [5, 50, 60], [0, 3, 7], [1, 2, 8], [0, 1, 2], [0, 30, 40], [20, 30, 40], [0, 1, 2]],
             served=[0, 0, 0, 1, 2, 3, 0, 0, 0])
    return Case(P, T, G, 9, log=log, speed=speed, **w)


ARRIVE = [2, 3, 4]      # the agents of hand_made() that arrive


# ---------------------------------------------------------------- the closed loop on the oracle
class RespawnOracleLoop(AH.AdmitOracleLoop):
    """AdmitOracleLoop with respawn at the end of every step: slot a serves the vehicles due[a][0..G-1]; the first goes through the gate with
    wait = due[a][0], every arrival is handed to `lib`'s rule -- the host build -- on this instance's words (no run log)."""

    def __init__(self, admit_lib, lib, paths, dl, start, due, gap, T=13, speed=False):
        due = _i32(due).reshape(len(paths), -1)
        super().__init__(admit_lib, paths, dl, start, wait=due[:, 0], gap=gap, T=T, speed=speed)
        A, G = self.A, due.shape[1]
        self.rlib, self.T = lib, T
        self.due, self.G = due, G
        self.served, self.steps_driven = _i32(np.zeros(A)), _i32(np.zeros(A))
        self.ep_i32, self.ep_f64 = _i32(np.zeros((A, G, 8))), _f64(np.zeros((A, G, 2)))
        self.start_state, self.start_idx = self.state.copy(), _i32(start)
        self.hits = 0

    def respawn(self):
        A, T = self.A, self.T
        u = np.stack([np.zeros((2, T)) if v is None else np.asarray(v, dtype=np.float64) for v in self.u]).reshape(A, 2 * T)
        prev = _i32(self.prev)
        case = Case(A, T, self.G, A, log=False, speed=self.speed, state=self.state, applied=self.applied, u=u, start_state=self.start_state,
                    traj_idx=self.traj_idx, target_ind=self.target, cut_len=np.zeros(A) if self.speed else prev, prev_len=prev if self.speed else np.zeros(A),
                    own=np.arange(A), done=np.array(self.done, dtype=np.int32), steps_driven=self.steps_driven, wait=self.wait, entered=self.entered,
                    clock=self.clock, start_idx=self.start_idx, due=self.due, served=self.served, ep_i32=self.ep_i32, ep_f64=self.ep_f64)
        before = case.served.copy()
        host_step(self.rlib, case)
        for a in np.flatnonzero(case.served != before):
            if case.wait[a] >= 0:           # reset: a fresh warm start
                self.u[a] = None
        self.state, self.applied = case.state, case.applied
        self.traj_idx, self.target = [int(v) for v in case.traj_idx], [int(v) for v in case.target_ind]
        self.prev = [int(v) for v in (case.prev_len if self.speed else case.cut_len)]
        self.steps_driven, self.wait, self.entered = case.steps_driven, case.wait, case.entered
        self.served, self.ep_i32, self.ep_f64 = case.served, case.ep_i32, case.ep_f64

    def step(self):
        out = super().step()
        for a in range(self.A):
            if out[a] is not None:
                self.steps_driven[a] += 1
                self.hits += int(out[a]['hit'] >= 0)
        self.respawn()
        return out

    def episodes(self, a):
        """[(entered, arrived, driven)] of slot a's finished episodes"""
        return [tuple(int(v) for v in self.ep_i32[a, g, :3]) for g in range(int(self.served[a]))]
