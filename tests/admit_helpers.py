"""Admission (mpcx_admit: agents enter the scene on a schedule) for the tests: the host build of csrc/mpcx_admit_core.h
(tests/admit_ref/admit_ref.cpp) behind numpy arrays, a numpy restatement of the rule, the hand-made pools that tests/test_admit_cpu.py runs
through the host build and tests/test_gpu_admit.py through the device stage, and the closed loop of several egos on the CPU oracle with
admission at the head of every step (AdmitOracleLoop)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import scene_helpers as SH

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'admit_ref', 'admit_ref.cpp')
INC = ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc')]
GONE, PRESENT, DUE = 0, 1, 2        # the tags of the table (mpcx_admit_core.h)


def build_ref(directory):
    """the host build as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    from mpc_for_av_at_intersection_amd import _lib
    so = os.path.join(str(directory), 'libadmit_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.admit_ref_step.restype = C.c_int
    lib.admit_ref_step.argtypes = ([C.POINTER(_lib.InteractionParamsC), C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 +
                                   [C.c_int64, C.c_void_p, C.POINTER(_lib.AdmitC), C.c_int] + [C.c_void_p] * 3)
    lib.admit_ref_actor_row.restype = None
    lib.admit_ref_actor_row.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.admit_ref_layout.restype = None
    return lib


def interaction_params(radius, centers):
    from mpc_for_av_at_intersection_amd import _lib
    ip = _lib.InteractionParamsC()
    ip.radius = radius
    ip.circle_centers[:] = list(np.asarray(centers, dtype=np.float64).ravel())
    return ip


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


class Case:
    """one pool with its agents, scripted cars and admission words, as numpy arrays (copies: a Case may be run more than once)"""

    def __init__(self, state, own, wait, done, absent, gap, radius=1.0, centers=(0.5, 0.0, 2.0, 0.0), obs_off=None, obs_cnt=None, clock=0,
                 entered=None, actors=None, actor_state=None, actor_row=None, tape=None):
        from mpc_for_av_at_intersection_amd import _lib
        self.state = np.ascontiguousarray(np.asarray(state, dtype=np.float64).reshape(-1, 4))
        P = self.P = len(self.state)
        self.own, self.wait, self.done, self.absent = _i32(own), _i32(wait), _i32(done), _i32(absent)
        self.n_pool = len(self.absent)
        self.obs_off = _i32(np.zeros(P) if obs_off is None else obs_off)
        self.obs_cnt = _i32(np.full(P, self.n_pool) if obs_cnt is None else obs_cnt)
        self.entered = _i32(np.where(self.wait >= 0, -1, 0) if entered is None else entered)
        self.clock = _i32([clock])
        self.gap, self.radius, self.centers = float(gap), float(radius), np.asarray(centers, dtype=np.float64).ravel()
        self.actors = np.zeros(0, _lib.TRAFFIC_ACTOR_DTYPE) if actors is None else np.ascontiguousarray(actors)
        self.actor_state = np.ascontiguousarray(np.asarray(np.zeros((0, 4)) if actor_state is None else actor_state, dtype=np.float64).reshape(-1, 4))
        self.actor_row = _i32([] if actor_row is None else actor_row)
        self.tape = None if tape is None else np.ascontiguousarray(np.asarray(tape, dtype=np.float64).reshape(-1, 6))

    def copy(self):
        return Case(self.state.copy(), self.own.copy(), self.wait.copy(), self.done.copy(), self.absent.copy(), self.gap, self.radius,
                    self.centers.copy(), self.obs_off.copy(), self.obs_cnt.copy(), int(self.clock[0]), self.entered.copy(), self.actors.copy(),
                    self.actor_state.copy(), self.actor_row.copy(), None if self.tape is None else self.tape.copy())

    def words(self):
        return dict(done=self.done.copy(), wait=self.wait.copy(), entered=self.entered.copy(), absent=self.absent.copy(), clock=int(self.clock[0]))

    def serialise(self, backwards, steps):
        """the record tests/admit_ref/admit_ref.cpp's main() reads"""
        head = np.array([self.P, self.n_pool, len(self.actors), 0 if self.tape is None else len(self.tape), int(backwards), steps], np.int32)
        dbl = np.concatenate([[self.gap, self.radius], self.centers])
        parts = [head, dbl, self.state, self.obs_off, self.obs_cnt, self.own, self.done, self.wait, self.entered, self.absent, self.clock, self.actors,
                 self.actor_state, self.actor_row] + ([] if self.tape is None else [self.tape])
        return b''.join(np.ascontiguousarray(p).tobytes() for p in parts)


def host_step(lib, case, backwards=False):
    """one step of the rule on `case`, in place, through the host build; returns dict(admitted, pose, tag, rows6)"""
    from mpc_for_av_at_intersection_amd import _lib
    ip = interaction_params(case.radius, case.centers)
    ad = _lib.AdmitC(case.wait.ctypes.data, case.entered.ctypes.data, case.clock.ctypes.data, 0, case.gap)
    pose, tag = np.full((case.n_pool, 3), np.nan), np.zeros(case.n_pool, np.int32)
    n = len(case.actors)
    rows6 = np.full((n, 6), np.nan)
    got = lib.admit_ref_step(C.byref(ip), case.P, case.state.ctypes.data, case.obs_off.ctypes.data, case.obs_cnt.ctypes.data, case.own.ctypes.data,
                             case.done.ctypes.data, case.n_pool, case.absent.ctypes.data, n, case.actors.ctypes.data if n else None,
                             case.actor_state.ctypes.data if n else None, None if case.tape is None else case.tape.ctypes.data,
                             0 if case.tape is None else len(case.tape), case.actor_row.ctypes.data if n else None, C.byref(ad), int(backwards),
                             pose.ctypes.data, tag.ctypes.data, rows6.ctypes.data if n else None)
    return dict(admitted=got, pose=pose, tag=tag, rows6=rows6)


def numpy_step(case, actor_rows=None):
    """The rule restated in numpy, in place on `case`: poses = the agents' state rows and the given get() rows of the actors (actor_rows,
    (n, 6)); a row blocks if it is present or the own row of a lower-numbered agent that is also due; clearance as
    tests/scene_helpers.clearance.  Returns the list of admitted agents."""
    n_pool = case.n_pool
    pose = np.full((n_pool, 6), np.nan)
    owner = np.full(n_pool, -1)
    before_absent, before_wait = case.absent.copy(), case.wait.copy()
    for q in range(case.P):
        if 0 <= case.own[q] < n_pool:
            pose[case.own[q], [0, 1, 3]] = case.state[q, [0, 1, 3]]
            owner[case.own[q]] = q
    known = owner >= 0
    for i, r in enumerate(case.actor_row):
        pose[r, [0, 1, 3]] = np.asarray(actor_rows)[i, [0, 1, 3]]
        known[r] = True
    admitted = []
    for q in range(case.P):
        if before_wait[q] > 0:
            case.wait[q] -= 1
        if before_wait[q] != 0 or not 0 <= case.own[q] < n_pool:
            continue
        own = int(case.own[q])
        window = [r for r in range(max(int(case.obs_off[q]), 0), min(int(case.obs_off[q]) + int(case.obs_cnt[q]), n_pool)) if r != own and known[r]]
        blocking = [r for r in window if before_absent[r] == 0 or (owner[r] >= 0 and owner[r] < q and before_wait[owner[r]] == 0)]
        if SH.clearance(pose, own, blocking, case.centers, case.radius) >= case.gap:
            admitted.append(q)
            case.done[q], case.absent[own], case.wait[q], case.entered[q] = 0, 0, -1, case.clock[0]
    case.clock[0] += 1
    return admitted


# ---------------------------------------------------------------- the hand-made pools (disc centres 0.5 and 2.0 m ahead of the pose, radius 1:
# two cars in line, d apart, have clearance d - 1.5 - 2)
def six_row_pool(d, gap=1.0):
    """Six rows, one window.  Agent 0 (row 0) drives at the origin.  Agent 1 (row 1) is DUE d metres behind it: clearance d - 3.5, so the
    threshold is d = 3.5 + gap.  Agent 2 (row 2) waits three more steps right beside agent 1 -- the NEAREST row, absent: it does not block.
    Agent 3 (row 3) has arrived and left (wait -1), on top of agent 1.  Agent 4 is due and names row 9, outside the pool.  Agent 5 (row 4)
    drives far away.  Row 5 is nobody's."""
    state = [[0.0, 0.0, 1.0, 0.0], [-d, 0.0, 0.0, 0.0], [-d, 0.5, 0.0, 0.0], [-d + 0.2, -0.3, 0.0, 0.1], [-d, 0.1, 0.0, 0.0], [40.0, 30.0, 2.0, 1.0]]
    return Case(state, own=[0, 1, 2, 3, 9, 4], wait=[-1, 0, 3, -1, 0, -1], done=[0, 1, 1, 1, 1, 0], absent=[0, 1, 1, 1, 0, 0], gap=gap, clock=7)


def tie_cases():
    """name -> (Case, agents admitted).  gap 0.5 throughout."""
    same = [3.0, -30.0, 0.0, np.pi / 2]
    far = [60.0, 10.0, 0.0, 0.0]
    beside = [3.0, -33.8, 0.0, np.pi / 2]       # 3.8 m behind `same`: clearance 0.3 < gap
    behind = [3.0, -37.6, 0.0, np.pi / 2]       # 3.8 m behind `beside`, 7.6 m behind `same`: clearance 4.1
    out = {}
    out['two at one pose'] = (Case([same, same], own=[0, 1], wait=[0, 0], done=[1, 1], absent=[1, 1], gap=0.5), [0])
    out['middle not due'] = (Case([same, same, same], own=[0, 1, 2], wait=[0, 2, 0], done=[1, 1, 1], absent=[1, 1, 1], gap=0.5), [0])
    out['judged against 0 only'] = (Case([far, same, same], own=[0, 1, 2], wait=[0, 2, 0], done=[1, 1, 1], absent=[1, 1, 1], gap=0.5), [0, 2])
    # agent 1 drives just ahead of where agent 0 wants to enter: 0 is held back, and still blocks 2, which is clear of everybody present
    out['priority whether or not it gets in'] = (Case([beside, same, behind, far], own=[1, 0, 2, 3], wait=[0, -1, 0, 0], done=[1, 0, 1, 1],
                                                      absent=[0, 1, 1, 1], gap=0.5), [3])
    return out


def actor_case(L=2.86):
    """agent 0 (row 0) due on the spawn pose of the stock scenario's second scripted car; a kinematic T-intersection car (row 1, the stock
    scenario's second one, six steps into its start delay... of 4 s: it stands) and a TAPE car (row 2) on its third row, 10 m away"""
    from mpc_for_av_at_intersection_amd import _lib
    from mpc_for_av_at_intersection_amd.batch import scripted_traffic_specs
    tr = scripted_traffic_specs(1, 2, 0, L)
    actors = np.zeros(2, _lib.TRAFFIC_ACTOR_DTYPE)
    actors[0] = tr.actors[1]
    actors[1]['kind'], actors[1]['tape_rows'], actors[1]['tape_off'], actors[1]['tape_stride'] = _lib.TRAFFIC_TAPE, 4, 1, 1
    tape = np.array([[0.0] * 6, [20.0, 3.0, 1.0, np.pi, 0.0, 0.0], [21.0, 3.0, 1.0, np.pi, 0.0, 0.0], [22.0, 3.0, 1.0, np.pi, 0.0, 0.01],
                     [23.0, 3.0, 1.0, np.pi, 0.0, 0.0], [99.0] * 6])
    actor_state = np.array([[30.0 - 0.125, 3.0, np.pi, 6.0], [0.0, 0.0, 0.0, 2.0]])
    return Case([[30.0, 3.0, 0.0, np.pi]], own=[0], wait=[0], done=[1], absent=[1, 0, 0], gap=0.0, actors=actors, actor_state=actor_state,
                actor_row=[1, 2], tape=tape)


# ---------------------------------------------------------------- the closed loop on the oracle
class AdmitOracleLoop(SH.OracleLoop):
    """OracleLoop with admission at the head of every step: agent a with wait[a] >= 0 waits outside the scene (done and absent) and is let
    in by `lib`'s rule -- the host build, called on this instance's pool: agents in rows 0 .. A - 1, one window over the whole pool."""

    def __init__(self, lib, paths, dl, start, wait, gap, T=13, speed=False):
        super().__init__(paths, dl, start, T=T, depart=True, speed=speed)
        A = self.A
        self.lib, self.gap = lib, float(gap)
        self.wait, self.clock = _i32(wait), _i32([0])
        self.entered = _i32(np.where(self.wait >= 0, -1, 0))
        self.entry_clearance = [None] * A
        for a in range(A):
            if self.wait[a] >= 0:
                self.done[a] = self.absent[a] = True

    def admit(self):
        A = self.A
        case = Case(self.state, own=np.arange(A), wait=self.wait, done=np.array(self.done, dtype=np.int32), absent=np.array(self.absent, dtype=np.int32),
                    gap=self.gap, radius=self.radius, centers=self.centers.ravel(), clock=int(self.clock[0]), entered=self.entered)
        host_step(self.lib, case)
        for a in range(A):
            if self.done[a] and not case.done[a]:
                pool = self.pool()
                self.entry_clearance[a] = SH.clearance(pool, a, [r for r in range(A) if r != a and not self.absent[r]], self.centers, self.radius)
            self.done[a], self.absent[a] = bool(case.done[a]), bool(case.absent[a])
        self.wait, self.entered, self.clock = case.wait, case.entered, case.clock

    def step(self):
        self.admit()
        return super().step()

    def run(self, n):
        hist = []
        for _ in range(n):
            if all(self.done) and not (self.wait >= 0).any():
                break
            hist.append(self.step())
        return hist
