"""Routes (mpcx_routes: every vehicle of a respawning slot takes its own route from its own start pose) for the tests: the host build of
csrc/mpcx_route_core.h (tests/route_ref/route_ref.cpp) behind numpy arrays, a numpy restatement of the rule and of the per-movement summary,
the hand-made words that tests/test_route_cpu.py runs through the host build and tests/test_gpu_route.py through the device stage, and the
closed loop of several egos on the CPU oracle with admission at the head and the routed respawn at the end of every step (RouteOracleLoop)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import respawn_helpers as RH

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'route_ref', 'route_ref.cpp')
INC = RH.INC
# the words the rule may write, in the order route_ref.cpp's main() writes them back
MUT_F64 = RH.MUT_F64
MUT_I32 = RH.MUT_I32 + ('path_off', 'path_len')
ROUTE_I32 = ('route_off', 'route_len', 'route_of', 'rstart_idx')       # read-only
SUMMARY_DTYPE = np.dtype([(n, '<i8') for n in ('count', 'contacts', 'delay_sum', 'steps_driven_sum')] + [('min_clearance', '<f8')])


def build_ref(directory):
    """the host build as a shared library (g++ -ffp-contract=off, as the other host builds of the rules)"""
    from mpc_for_av_at_intersection_amd import _lib
    so = os.path.join(str(directory), 'libroute_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall'] + INC + ['-o', so, SRC], check=True)
    lib = C.CDLL(so)
    lib.route_ref_step.restype = C.c_int
    lib.route_ref_step.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 9 + [C.POINTER(_lib.RunLogC), C.POINTER(_lib.RetireC), C.POINTER(_lib.AdmitC),
                                                                   C.POINTER(_lib.RespawnC), C.POINTER(_lib.RoutesC), C.c_int])
    lib.route_ref_summary.restype = None
    lib.route_ref_summary.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
    lib.route_ref_layout.restype = None
    return lib


class Case(RH.Case):
    """respawn_helpers.Case plus the routes: route_off, route_len (R), route_of, rstart_idx (P, G), rstart_state (P, G, 4) and the words the
    routed reset also writes, path_off and path_len (P)"""

    def __init__(self, P, T, G, n_pool, R, log=True, speed=False, **words):
        super().__init__(P, T, G, n_pool, log=log, speed=speed, **words)
        self.R = int(R)
        shapes = dict(route_off=(R,), route_len=(R,), route_of=(P, G), rstart_idx=(P, G), path_off=(P,), path_len=(P,))
        for k, shape in shapes.items():
            setattr(self, k, RH._i32(words[k] if k in words else np.zeros(shape)).reshape(shape).copy())
        self.rstart_state = RH._f64(words['rstart_state'] if 'rstart_state' in words else np.zeros((P, G, 4))).reshape(P, G, 4).copy()

    def _all(self):
        return {k: getattr(self, k) for k in RH.MUT_F64 + RH.MUT_I32 + RH.CONST_I32 + ('start_state',) + ROUTE_I32 + ('path_off', 'path_len', 'rstart_state')}

    def copy(self):
        return Case(self.P, self.T, self.G, self.n_pool, self.R, self.log, self.speed, **self._all())

    def plain(self):
        """the same words without the routes: a respawn_helpers.Case"""
        return RH.Case(self.P, self.T, self.G, self.n_pool, self.log, self.speed,
                       **{k: getattr(self, k) for k in RH.MUT_F64 + RH.MUT_I32 + RH.CONST_I32 + ('start_state',)})

    def words(self):
        return {k: getattr(self, k).copy() for k in MUT_F64 + MUT_I32}

    def blob(self):
        """the mutable words as route_ref.cpp's main() writes them back (without the count of arrivals)"""
        return b''.join(getattr(self, k).tobytes() for k in MUT_F64 + MUT_I32)

    def serialise(self, backwards, steps):
        """the record tests/route_ref/route_ref.cpp's main() reads"""
        plain = super().serialise(backwards, steps)
        tail = b''.join(getattr(self, k).tobytes() for k in ('route_off', 'route_len', 'route_of', 'rstart_idx', 'path_off', 'path_len', 'rstart_state'))
        return plain[:32] + np.int32(self.R).tobytes() + plain[32:] + tail


def structs(case, ptr=lambda a: a.ctypes.data):
    """(RunLogC or None, RetireC, AdmitC, RespawnC, RoutesC) naming the arrays of `case` (ptr: array -> address)"""
    from mpc_for_av_at_intersection_amd import _lib
    rt = _lib.RoutesC(case.R, 0, ptr(case.route_off), ptr(case.route_len), ptr(case.route_of), ptr(case.rstart_state), ptr(case.rstart_idx),
                      ptr(case.path_off), ptr(case.path_len))
    return RH.structs(case, ptr) + (rt,)


def host_step(lib, case, backwards=False):
    """one step of the rule on `case`, in place, through the host build; returns the number of agents that arrived"""
    log, retire, admit, rs, rt = structs(case)
    return lib.route_ref_step(case.P, case.n_pool, 2 * case.T, case.state.ctypes.data, case.applied.ctypes.data, case.u.ctypes.data,
                              case.traj_idx.ctypes.data, case.target_ind.ctypes.data, case.cut_len.ctypes.data, case.iters.ctypes.data,
                              case.prev_len.ctypes.data if case.speed else None, case.own.ctypes.data,
                              None if log is None else C.byref(log), C.byref(retire), C.byref(admit), C.byref(rs), C.byref(rt), int(backwards))


def numpy_step(c):
    """The rule restated in numpy, in place on `c`: the respawn rule (respawn_helpers.numpy_step), then, per arrival, the episode's route
    word and -- if the slot was reset -- the next vehicle's pose, index and route, or the never-driven state for a defective one.  Returns
    the list of agents that arrived."""
    g0 = c.served.copy()
    arrived = RH.numpy_step(c)
    for q in arrived:
        g = int(g0[q])
        c.ep_i32[q, g, 7] = c.route_of[q, g]
        if g + 1 >= c.G:
            continue
        r, s = int(c.route_of[q, g + 1]), int(c.rstart_idx[q, g + 1])
        if not 0 <= r < c.R or not 0 <= s < c.route_len[r]:
            c.wait[q] = c.entered[q] = -1
            continue
        c.state[q] = c.rstart_state[q, g + 1]
        c.traj_idx[q] = c.target_ind[q] = s
        c.path_off[q], c.path_len[q] = c.route_off[r], c.route_len[r]
    return arrived


def summary_numpy(A, R, served, ep_i32, ep_f64):
    """mpcx_episode_summary restated in numpy -- THE definition: per instance b (A consecutive slots) and route r, over the finished episodes
    (g < served[q]) whose word 7 is r: their number, the number with contact_step (word 4) >= 0, the sum of entered - due (words 0 and 6), the
    sum of steps_driven (word 2) and the minimum of min_clearance (+inf if there are none).  Returns a (B, R) array of SUMMARY_DTYPE."""
    served, w, f = np.asarray(served), np.asarray(ep_i32).astype(np.int64), np.asarray(ep_f64)
    P, G = w.shape[:2]
    out = np.zeros((P // A, R), SUMMARY_DTYPE)
    out['min_clearance'] = np.inf
    for q in range(P):
        for g in range(min(int(served[q]), G)):
            r = int(w[q, g, 7])
            if not 0 <= r < R:
                continue
            o = out[q // A, r]
            o['count'] += 1
            o['contacts'] += int(w[q, g, 4] >= 0)
            o['delay_sum'] += w[q, g, 0] - w[q, g, 6]
            o['steps_driven_sum'] += w[q, g, 2]
            o['min_clearance'] = min(o['min_clearance'], f[q, g, 0])
    return out


def host_summary(lib, A, R, served, ep_i32, ep_f64):
    """the same table through the host build (the loop the device kernel strides over, one record at a time)"""
    served, w, f = RH._i32(served), RH._i32(ep_i32), RH._f64(ep_f64)
    P, G = w.shape[:2]
    oi, of = np.zeros((P // A, R, 4), np.int64), np.zeros((P // A, R))
    lib.route_ref_summary(P, A, G, R, served.ctypes.data, w.ctypes.data, f.ctypes.data, oi.ctypes.data, of.ctypes.data)
    out = np.zeros((P // A, R), SUMMARY_DTYPE)
    for k, n in enumerate(SUMMARY_DTYPE.names[:4]):
        out[n] = oi[..., k]
    out['min_clearance'] = of
    return out


# ---------------------------------------------------------------- the hand-made words
ARRIVE = [2, 3, 4, 5, 6]    # the agents of hand_made() that arrive
RESET = [2, 3]              # ... whose slot is reset onto its next vehicle's route
DEFECT = [5, 6]             # ... whose next vehicle is defective
R_HAND = 3


def hand_made(log=True, speed=False, seed=7, P=9):
    """respawn_helpers.hand_made (nine agents, G = 3, the clock at 20) with three routes of 700, 800 and 650 points at path points 0, 700
    and 1500, a route, a start pose and a start index per vehicle, and path_off / path_len words that hold something else before.  Agents 5
    and 6 -- finished / own row outside the pool there -- arrive here with served 0: the next vehicle of 5 has route index R (= 3), that of 6
    starts at index route_len (= 800 on route 1): both defective.  So: 0 driving, 1 waiting, 2 and 3 reset onto the next vehicle's route,
    4 the last vehicle of its slot, 5 and 6 never driven again, 7 due, 8 never entered.
    P > 9: the nine agents repeated until there are P (every agent has its own pool row)."""
    base = RH.hand_made(log, speed, seed)
    rng = np.random.default_rng(seed + 1)
    n, P, G = int(P), base.P, base.G
    w = {k: getattr(base, k) for k in RH.MUT_F64 + RH.MUT_I32 + RH.CONST_I32 + ('start_state',)}
    w['served'] = np.array([0, 0, 0, 1, 2, 0, 0, 0, 0], np.int32)
    w['own'] = np.arange(P, dtype=np.int32)
    route_len = np.array([700, 800, 650], np.int32)
    route_of = rng.integers(0, R_HAND, (P, G)).astype(np.int32)
    route_of[2, 1], route_of[3, 2] = 2, 1       # the routes the two resets move to
    route_of[5, 1] = R_HAND
    route_of[6, 1] = 1
    rstart_idx = rng.integers(0, 600, (P, G)).astype(np.int32)
    rstart_idx[6, 1] = 800
    w.update(route_off=[0, 700, 1500], route_len=route_len, route_of=route_of, rstart_idx=rstart_idx, rstart_state=rng.normal(size=(P, G, 4)),
             path_off=5000 + np.arange(P), path_len=100 + np.arange(P))
    if n != P:
        for k, v in list(w.items()):
            if k not in ('clock', 'route_off', 'route_len'):
                w[k] = np.concatenate([np.asarray(v).reshape(P, -1)] * (-(-n // P)))[:n]
        w['own'] = np.arange(n, dtype=np.int32)
    return Case(n, base.T, G, n, R_HAND, log=log, speed=speed, **w)


# ---------------------------------------------------------------- the closed loop on the oracle
class RouteOracleLoop(RH.RespawnOracleLoop):
    """RespawnOracleLoop with a route per vehicle: slot a serves vehicle g on routes[route_of[a][g]] from index start_idx[a][g] (v0 = 0);
    every arrival is handed to `lib`'s rule -- the host build of mpcx_route_core.h -- on this instance's words (no run log), and a slot
    whose path_off word changed drives the route it names from then on."""

    def __init__(self, admit_lib, lib, routes, dl, route_of, start_idx, due, gap, T=13, speed=False):
        route_of, start_idx = RH._i32(route_of), RH._i32(start_idx)
        A, G = route_of.shape
        super().__init__(admit_lib, None, [routes[r] for r in route_of[:, 0]], dl, [int(s) for s in start_idx[:, 0]], due, gap, T=T, speed=speed)
        assert self.G == G
        self.paths = list(self.paths)
        self.routes, self.route_lib = routes, lib
        lens = np.array([len(r) for r in routes])
        self.route_off, self.route_len = RH._i32(np.cumsum(np.concatenate([[0], lens[:-1]]))), RH._i32(lens)
        self.route_of, self.rstart_idx = route_of, start_idx
        self.rstart_state = np.zeros((A, G, 4))
        for a in range(A):
            for g in range(G):
                p = routes[route_of[a, g]][start_idx[a, g]]
                self.rstart_state[a, g] = [p[0], p[1], 0.0, p[2]]
        self.path_off, self.path_len = self.route_off[route_of[:, 0]].copy(), self.route_len[route_of[:, 0]].copy()

    def respawn(self):
        A, T = self.A, self.T
        u = np.stack([np.zeros((2, T)) if v is None else np.asarray(v, dtype=np.float64) for v in self.u]).reshape(A, 2 * T)
        prev = RH._i32(self.prev)
        case = Case(A, T, self.G, A, len(self.routes), log=False, speed=self.speed, state=self.state, applied=self.applied, u=u,
                    start_state=self.start_state, traj_idx=self.traj_idx, target_ind=self.target, cut_len=np.zeros(A) if self.speed else prev,
                    prev_len=prev if self.speed else np.zeros(A), own=np.arange(A), done=np.array(self.done, dtype=np.int32),
                    steps_driven=self.steps_driven, wait=self.wait, entered=self.entered, clock=self.clock, start_idx=self.start_idx, due=self.due,
                    served=self.served, ep_i32=self.ep_i32, ep_f64=self.ep_f64, route_off=self.route_off, route_len=self.route_len,
                    route_of=self.route_of, rstart_idx=self.rstart_idx, rstart_state=self.rstart_state, path_off=self.path_off,
                    path_len=self.path_len)
        before = case.served.copy()
        host_step(self.route_lib, case)
        for a in np.flatnonzero(case.served != before):
            if case.wait[a] >= 0:           # reset: a fresh warm start, on the route its words now name
                self.u[a] = None
                self.paths[a] = self.routes[int(np.flatnonzero(self.route_off == case.path_off[a])[0])]
                assert len(self.paths[a]) == case.path_len[a]
        self.state, self.applied = case.state, case.applied
        self.traj_idx, self.target = [int(v) for v in case.traj_idx], [int(v) for v in case.target_ind]
        self.prev = [int(v) for v in (case.prev_len if self.speed else case.cut_len)]
        self.steps_driven, self.wait, self.entered = case.steps_driven, case.wait, case.entered
        self.served, self.ep_i32, self.ep_f64 = case.served, case.ep_i32, case.ep_f64
        self.path_off, self.path_len = case.path_off, case.path_len
