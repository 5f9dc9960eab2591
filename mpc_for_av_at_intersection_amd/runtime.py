"""Thin device runtime over the C ABI (include/mpcx.h): torch-ROCm tensors own the device buffers, every
computation happens in libmpcx.so's HIP kernels.  No CPU fallback exists: constructing a Context without a
GPU or without the built library raises."""
import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Tuple, Optional, Sequence

import numpy as np
import torch

from . import _lib


@dataclass
class MpcParams:
    """main/config/mpc_config.json + lib/mpc.py:17-36 + lib/simulation.py:23-25 of the reference."""
    T: int = 13
    dt: float = 0.2
    L: float = 2.86
    w_perp: float = 20.0
    w_para: float = 1.0
    R: Sequence[float] = (0.01, 0.01)
    Rd: Sequence[float] = (0.01, 1.0)
    Q_v_yaw: Sequence[float] = (0.0, 0.5)
    Qf_base: Sequence[float] = (1.0, 1.0, 0.0, 0.5)   # multiplied by T (mpc.py:25)
    R_end: Sequence[float] = (10.0, 10.0)
    max_speed: float = 30.0 / 3.6
    min_speed: float = -5.0
    max_accel: float = 2.0
    max_decel: float = -10.0
    max_steer: float = float(np.deg2rad(45.0))
    max_dsteer: float = float(np.deg2rad(30.0))
    max_iter: int = 60
    tol: float = 1e-10
    model: int = _lib.MODEL_BICYCLE4     # _lib.MODEL_JERK5: the five-state problem of lib/mpc_jerk.py
    jerk_weight: float = 1.0             # jerk_penalty_weight, mpc_jerk.py:30

    @classmethod
    def jerk(cls, **kw) -> 'MpcParams':
        """the constants of main/lib/mpc_jerk.py:16-39: T 13, cross-track weight 10 (line 167), Rd (0.3, 1), MAX_DECEL -5"""
        base = dict(T=13, w_perp=10.0, w_para=1.0, R=(0.01, 0.01), Rd=(0.3, 1.0), Q_v_yaw=(0.0, 0.5),
                    Qf_base=(1.0, 1.0, 0.0, 0.5), max_accel=2.0, max_decel=-5.0, model=_lib.MODEL_JERK5, jerk_weight=1.0)
        base.update(kw)
        return cls(**base)

    def to_c(self) -> _lib.MpcParamsC:
        p = _lib.MpcParamsC()
        p.T, p.max_iter, p.dt, p.L = int(self.T), int(self.max_iter), float(self.dt), float(self.L)
        p.w_perp, p.w_para = float(self.w_perp), float(self.w_para)
        p.R[:] = list(map(float, self.R)); p.Rd[:] = list(map(float, self.Rd))
        p.Q_v_yaw[:] = list(map(float, self.Q_v_yaw))
        p.Qf[:] = [float(q) * self.T for q in self.Qf_base]
        p.R_end[:] = list(map(float, self.R_end))
        p.max_speed, p.min_speed = float(self.max_speed), float(self.min_speed)
        p.max_accel, p.max_decel = float(self.max_accel), float(self.max_decel)
        p.max_steer, p.max_dsteer, p.tol = float(self.max_steer), float(self.max_dsteer), float(self.tol)
        p.model, p.reserved, p.jerk_weight = int(self.model), 0, float(self.jerk_weight)
        return p

    def tuning_row(self) -> np.ndarray:
        """the 16 doubles of mpcx_qp_tuning (include/mpcx.h) for this parameter set"""
        return np.array([self.w_perp, self.w_para, *self.R, *self.Rd, *self.Q_v_yaw, *[float(q) * self.T for q in self.Qf_base],
                         self.max_accel, self.max_decel, self.max_dsteer, 0.0], dtype=np.float64)


@dataclass
class InteractionParams:
    """scenario constants of main/scenarios/mpc_intersection.py:31,81-84 + car_dimensions.py"""
    pred_steps: int = 35
    frame_window: int = 20
    cutoff_margin: int = 72
    dt: float = 0.2
    L: float = 2.86
    radius: float = 2.0 / 2 ** 0.5
    circle_centers: Sequence[float] = (2.18, 0.0, 0.68, 0.0)
    max_accel: float = 2.0
    max_speed: float = 30.0 / 3.6
    max_path_len: int = 0        # longest path of the batch in points (0 = the kernel's default capacity of 1024)
    path_cum: Optional[torch.Tensor] = None    # per point of the path table: arc length from the start of its path (device, float64) ...
    path_cum_err: float = 0.0                  # ... and the bound on the error of its differences (see mpcx_interaction_params; `path_tables()`)
    path_first_within: Optional[torch.Tensor] = None   # per point: first point of its path within 1 mm of it (device, int32; `path_first_within()`)
    plan: Optional[dict] = None                # ego prediction per path point (`path_plan()` uploaded: cnt, disc, box, path_disc tensors + cap, steps, dl, radius)

    def to_c(self) -> _lib.InteractionParamsC:
        p = _lib.InteractionParamsC()
        p.pred_steps, p.frame_window, p.cutoff_margin, p.max_path_len = int(self.pred_steps), int(self.frame_window), int(self.cutoff_margin), int(self.max_path_len)
        p.dt, p.L, p.radius = float(self.dt), float(self.L), float(self.radius)
        cc = list(map(float, np.asarray(self.circle_centers, dtype=np.float64).ravel()))
        if len(cc) == 2:
            # car_dimensions.py:51-75 with skip_back_circle_collision_checking=True: ONE disc.  The kernels test two; the same disc twice
            # gives the reference's one-disc answers (every test is a min / first-hit over the discs, and the frame index is taken
            # modulo the path length, collision_avoidance.py:92-98)
            cc = cc + cc
        if len(cc) != 4:
            raise MpcxError('car_dimensions.circle_centers must hold one or two discs (x, y offsets), got %d numbers' % len(cc))
        p.circle_centers[:] = cc
        p.max_accel, p.max_speed = float(self.max_accel), float(self.max_speed)
        p.path_cum = None if self.path_cum is None else C.c_void_p(self.path_cum.data_ptr())
        p.path_cum_err = float(self.path_cum_err) if self.path_cum is not None else 0.0
        p.path_first_within = None if self.path_first_within is None else C.c_void_p(self.path_first_within.data_ptr())
        if self.plan is not None and self.path_cum is not None:
            pl = self.plan
            p.plan_cnt, p.plan_disc, p.plan_box, p.path_disc = (C.c_void_p(pl[k].data_ptr()) for k in ('cnt', 'disc', 'box', 'path_disc'))
            p.plan_cap, p.plan_steps, p.plan_dl, p.plan_radius = int(pl['cap']), int(pl['steps']), float(pl['dl']), float(pl['radius'])
        return p


class MpcxError(RuntimeError):
    pass


def path_tables(table: np.ndarray, offs) -> Tuple[np.ndarray, float]:
    """Arc-length table for mpcx_interaction_params.path_cum: for the concatenated path table `table` ((n, >= 2): x, y, ...) whose
    paths start at offs[0], offs[1], ... (offs[-1] = n), per point the running sum of the step lengths of ITS path (np.cumsum, restarted
    per path) and the bound on the distance between a difference of two entries and the reference's own running sum over the same steps
    (trajectories.py:72-79): both are sequential float64 sums of at most n_max non-negative terms adding up to at most L, each within
    (n_max - 1) * 2^-53 * L of the exact sum (first-order bound, doubled here), plus one rounding of the subtraction."""
    table = np.asarray(table, dtype=np.float64)
    cum = np.zeros(len(table))
    worst = 0.0
    for a, b in zip(offs[:-1], offs[1:]):
        if b - a < 1:
            continue
        d = table[a + 1:b, :2] - table[a:b - 1, :2]
        steps = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        cum[a + 1:b] = np.cumsum(steps)
        n, length = b - a, float(cum[b - 1]) if b - a > 1 else 0.0
        worst = max(worst, 2.0 * (3 * n + 2) * 2.0 ** -53 * length)
    return cum, worst


def path_first_within(table: np.ndarray, offs, radius: float = 0.001) -> np.ndarray:
    """mpcx_interaction_params.path_first_within: for every point k of the concatenated path table (paths start at offs[0], offs[1], ...,
    offs[-1] = n) the index, relative to its path's first point, of the first point j <= k of the same path with
    np.linalg.norm(p_j - p_k) <= radius -- what get_cutoff_curve_by_position_idx(path, *p_k[:2]) returns (collision_avoidance.py:107-119),
    with the reference's own numpy expression."""
    table = np.asarray(table, dtype=np.float64)
    out = np.zeros(len(table), dtype=np.int32)
    for a, b in zip(offs[:-1], offs[1:]):
        pts = table[a:b, :2]
        for k0 in range(0, b - a, 256):                     # (k, j) blocks of 256 x n: bounded memory for long paths
            k1 = min(k0 + 256, b - a)
            diff = pts[None, :, :] - pts[k0:k1, None, :]      # points_diff[:, 0] -= x; points_diff[:, 1] -= y
            near = np.linalg.norm(diff, axis=2) <= radius
            out[a + k0:a + k1] = np.argmax(near, axis=1)     # first True; the point itself is always one
    return out


def path_plan(table: np.ndarray, cs: np.ndarray, offs, dt: float, max_speed: float, circle_centers, radius: float, pred_steps: int,
              cap: int = 64, n_runs: int = 8) -> dict:
    """mpcx_interaction_params.plan_*: for every point t of the concatenated path table the ego prediction the scenario loop builds from
    trajectory_full[t:] once the predicted speed has saturated (mpc_intersection.py:107-116: resample_curve with dl = DT * MAX_SPEED),
    evaluated with the reference's own numpy expressions: which poses are kept (trajectories.py:58-86, np.cumsum restarted at t), their
    disc centres (trajectories.py:11-37 with the host's cos / sin of the yaw column) and, for the conflict search's cull, the bounding
    boxes of `n_runs` runs of frames of the padded prediction (max(kept, pred_steps) frames), inflated by a little more than 2 * radius.
    Returns numpy arrays cnt (npts,), disc (npts, cap, 4), box (npts, n_runs, 4), path_disc (npts, 4) + cap, steps, dl, radius."""
    table = np.asarray(table, dtype=np.float64)
    cs = np.asarray(cs, dtype=np.float64)
    npts = len(table)
    cc = np.asarray(circle_centers, dtype=np.float64).reshape(-1, 2)
    if len(cc) == 1:
        cc = np.repeat(cc, 2, axis=0)
    c, s = cs[:, 0], cs[:, 1]
    path_disc = np.empty((npts, 4))
    for d in range(2):
        path_disc[:, 2 * d] = (c * cc[d, 0] - s * cc[d, 1]) + table[:, 0]
        path_disc[:, 2 * d + 1] = (s * cc[d, 0] + c * cc[d, 1]) + table[:, 1]
    dl = dt * max_speed
    md = 2.0 * radius
    slack = md * (1.0 + 1e-9) + 1e-9
    cnt = np.zeros(npts, dtype=np.int32)
    disc = np.zeros((npts, cap, 4))
    box = np.empty((npts, n_runs, 4))
    box[:, :, 0::2] = np.inf; box[:, :, 1::2] = -np.inf
    for a, b in zip(offs[:-1], offs[1:]):
        if b - a < 1:
            continue
        seg = np.append(0.0, np.linalg.norm(table[a + 1:b, :2] - table[a:b - 1, :2], axis=1))      # seg[i]: step into point i of the path
        for t in range(a, b):
            steps = seg[t - a:].copy()
            steps[0] = 0.0                                  # np.append(0., norm(diff)) of the sub-path starting at t
            bucket = np.floor(steps.cumsum() / dl).astype(int)
            keep = np.append(True, (bucket[1:] - bucket[:-1]) >= 1.)
            keep[-1] = True
            idx = np.nonzero(keep)[0]
            k = len(idx)
            if k > cap:
                continue                                    # not tabulated: the kernel resamples
            cnt[t] = k
            ego = path_disc[t + idx]
            disc[t, :k] = ego
            F = max(k, pred_steps)
            SL = (F + n_runs - 1) // n_runs
            padded = ego[np.minimum(np.arange(F), k - 1)]   # frames beyond the prediction repeat its last pose
            for sg in range(n_runs):
                run = padded[sg * SL:(sg + 1) * SL]
                if len(run):
                    xs, ys = run[:, 0::2], run[:, 1::2]
                    box[t, sg] = (xs.min() - slack, xs.max() + slack, ys.min() - slack, ys.max() + slack)
    return dict(cnt=cnt, disc=disc, box=box, path_disc=path_disc, cap=cap, steps=int(pred_steps), dl=dl, radius=float(radius))


def traffic_pool_layout(B: int, A: int, k_of_instance, a_lo: int = 0, a_total: Optional[int] = None) -> dict:
    """The obstacle pool of a batch of B instances x A agents with k_of_instance[b] scripted actors in instance b: every instance owns
    stride = a_total + max(K) consecutive rows, [its agents | its actors | unused], so that the window of each of its agents --
    obs_off = b * stride, obs_cnt = a_total + K_b, obs_skip = the agent's own row -- stays ONE contiguous run (what
    mpcx_interaction_batch takes).  Returns int32 arrays obs_off / obs_cnt / obs_skip / ego_row (per agent, (instance, agent) order),
    actor_row (per actor, (instance, actor) order) + stride, pool_rows.  Raises ValueError where an agent would see more than
    MPCX_MAX_OBS moving obstacles.  (a_lo, a_total: the agent-sharded layout's part of the agents; without traffic only.)"""
    k = np.asarray(k_of_instance, dtype=np.int64).reshape(-1)
    a_total = A if a_total is None else int(a_total)
    if len(k) != B or (k < 0).any():
        raise ValueError('traffic: one non-negative actor count per instance expected, got %d for %d instances' % (len(k), B))
    kmax = int(k.max()) if B else 0
    if B and a_total - 1 + kmax > _lib.MAX_OBS:
        raise ValueError('an agent would see %d other agents + %d scripted actors: more than MPCX_MAX_OBS = %d moving obstacles'
                         % (a_total - 1, kmax, _lib.MAX_OBS))
    stride = a_total + kmax
    inst = np.repeat(np.arange(B), A)
    agent = np.tile(np.arange(A), B) + a_lo
    ego_row = inst * stride + agent
    actor_inst = np.repeat(np.arange(B), k)
    actor_k = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(stride=stride, pool_rows=B * stride, obs_off=i32(inst * stride), obs_cnt=i32(a_total + k[inst]), obs_skip=i32(ego_row),
                ego_row=i32(ego_row), actor_row=i32(actor_inst * stride + a_total + actor_k))


class Traffic:
    """Scripted traffic of a batch (host side): the actor table (records of _lib.TRAFFIC_ACTOR_DTYPE = mpcx_traffic_actor, ordered by
    instance, then actor), the actors' start states (n, 4: x, y, theta, counter / cursor), how many actors each instance has, and the
    uploaded table TAPE actors read.  batch.IntersectionBatch(traffic=...) uploads it and steps it on the device."""

    def __init__(self, actors: np.ndarray, state: np.ndarray, k_of_instance, tape: Optional[np.ndarray] = None):
        self.actors = np.ascontiguousarray(actors, dtype=_lib.TRAFFIC_ACTOR_DTYPE).reshape(-1)
        self.state = np.ascontiguousarray(state, dtype=np.float64).reshape(-1, 4)
        self.k_of_instance = np.asarray(k_of_instance, dtype=np.int64).reshape(-1)
        self.tape = None if tape is None else np.ascontiguousarray(tape, dtype=np.float64).reshape(-1, 6)
        if len(self.actors) != len(self.state) or int(self.k_of_instance.sum()) != len(self.actors):
            raise ValueError('traffic: %d actors, %d states, %d actors counted over the instances'
                             % (len(self.actors), len(self.state), int(self.k_of_instance.sum())))

    @property
    def n_actors(self) -> int:
        return len(self.actors)

    @classmethod
    def empty(cls, B: int) -> 'Traffic':
        return cls(np.zeros(0, _lib.TRAFFIC_ACTOR_DTYPE), np.zeros((0, 4)), np.zeros(B, np.int64))

    @classmethod
    def from_specs(cls, specs_of_instance) -> 'Traffic':
        """specs_of_instance: per instance a list of `device_spec()` dicts (lib/moving_obstacles.py)"""
        flat = [s for inst in specs_of_instance for s in inst]
        actors = np.zeros(len(flat), _lib.TRAFFIC_ACTOR_DTYPE)
        for name in _lib.TRAFFIC_ACTOR_DTYPE.names:
            actors[name] = [s[name] for s in flat]
        state = np.array([s['state'] for s in flat], dtype=np.float64).reshape(-1, 4)
        return cls(actors, state, [len(inst) for inst in specs_of_instance])

    @classmethod
    def from_objects(cls, vehicles_of_instance) -> 'Traffic':
        """per instance a list of scripted vehicles (lib.moving_obstacles.MovingObstacle*), taken in their CURRENT state"""
        return cls.from_specs([[o.device_spec() for o in inst] for inst in vehicles_of_instance])

    @classmethod
    def from_tapes(cls, tapes, track_of_instance) -> 'Traffic':
        """TAPE actors: tapes = list of (n_t, K_t, 6) arrays (track t: n_t steps of K_t vehicles, rows as get() returns them -- e.g.
        np.stack([o.tape(n) for o in vehicles], axis=1) or recorded traffic); instance b replays track track_of_instance[b] with one actor
        per vehicle, from row 0, holding the last row once the track has ended.  Tracks are uploaded once, whatever the number of
        instances that play them."""
        tapes = [np.ascontiguousarray(t, dtype=np.float64) for t in tapes]
        for t in tapes:
            if t.ndim != 3 or t.shape[2] != 6 or t.shape[0] < 1:
                raise ValueError('traffic: a tape track has shape (steps >= 1, vehicles, 6), got %s' % (t.shape,))
        off = np.cumsum([0] + [t.shape[0] * t.shape[1] for t in tapes])
        track = np.asarray(track_of_instance, dtype=np.int64).reshape(-1)
        k = np.array([tapes[t].shape[1] for t in track], dtype=np.int64)
        actors = np.zeros(int(k.sum()), _lib.TRAFFIC_ACTOR_DTYPE)
        which = np.repeat(track, k)
        lane = np.arange(len(actors)) - np.repeat(np.cumsum(k) - k, k)
        actors['kind'] = _lib.TRAFFIC_TAPE
        actors['direction'] = 1
        actors['tape_rows'] = [tapes[t].shape[0] for t in which]
        actors['tape_off'] = off[which] + lane
        actors['tape_stride'] = [tapes[t].shape[1] for t in which]
        table = np.concatenate([t.reshape(-1, 6) for t in tapes]) if tapes else np.zeros((0, 6))
        state = np.zeros((len(actors), 4))
        if len(actors):
            state[:, :3] = table[actors['tape_off']][:, [0, 1, 3]]
        return cls(actors, state, k, tape=table)

    def slice(self, lo: int, hi: int) -> 'Traffic':
        """the traffic of instances lo .. hi-1 (instance-sharded runs)"""
        first = np.concatenate([[0], np.cumsum(self.k_of_instance)])
        a, b = int(first[lo]), int(first[hi])
        return Traffic(self.actors[a:b], self.state[a:b], self.k_of_instance[lo:hi], tape=self.tape)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ordered(fn):
    """Every launch goes to the CONTEXT's stream.  When that is not torch's current stream (a Context created on a stream of its
    own while the caller's tensors are produced and consumed on another), the call is ordered on both sides: the context's stream
    first waits for what the current stream has queued (the inputs), and the current stream afterwards waits for the launch (the
    outputs; that also keeps the caching allocator from handing a buffer back while a kernel still uses it).  Two event
    operations, and nothing at all in the default case of one shared stream."""
    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        cur = torch.cuda.current_stream(self.device)
        if cur == self.stream:
            return fn(self, *a, **k)
        self.stream.wait_stream(cur)
        try:
            return fn(self, *a, **k)
        finally:
            cur.wait_stream(self.stream)
    return wrapped


class Context:
    """One mpcx_ctx bound to a torch device and (by default) torch's current stream on it.  A Context on a stream of its own may be
    used from any current stream: see _ordered."""

    def __init__(self, device: int = 0, stream: Optional[torch.cuda.Stream] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise MpcxError('no GPU visible: the mpcx hot path is HIP-only (no CPU fallback)')
        self.device = torch.device('cuda', device)
        torch.cuda.set_device(self.device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._ctx = self.lib.mpcx_create(device, C.c_void_p(self.stream.cuda_stream))
        if not self._ctx:
            raise MpcxError('mpcx_create failed for device %d' % device)
        self.params: Optional[MpcParams] = None

    def close(self):
        if getattr(self, '_ctx', None):
            self.lib.mpcx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MpcxError('mpcx error %d: %s' % (rc, self.lib.mpcx_last_error(self._ctx).decode()))

    # ------------------------------------------------------------------ helpers
    def f64(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

    def i32(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def u8(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8)).to(self.device)

    def _want(self, t, dtype, shape=None, name='tensor'):
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise MpcxError('%s must be a contiguous %s tensor on %s' % (name, dtype, self.device))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise MpcxError('%s has shape %s, expected %s' % (name, tuple(t.shape), tuple(shape)))
        return t

    # ------------------------------------------------------------------ entry points
    def set_mpc_params(self, p: MpcParams):
        cp = p.to_c()
        self._chk(self.lib.mpcx_set_mpc_params(self._ctx, C.byref(cp)))
        self.params = p

    @_ordered
    def qp_solve(self, x0, xref, xbar, reaches_end, u_warm=None, out=None):
        """mpcx_qp_solve_batch. Returns dict(x (B,4,T+1), u (B,2,T), status, iters, kkt)."""
        T = self.params.T
        B = x0.shape[0]
        f = torch.float64
        self._want(x0, f, (B, 4), 'x0'); self._want(xref, f, (B, 4, T + 1), 'xref')
        self._want(xbar, f, (B, 4, T + 1), 'xbar'); self._want(reaches_end, torch.uint8, (B, T + 1), 'reaches_end')
        if u_warm is not None:
            self._want(u_warm, f, (B, 2, T), 'u_warm')
        if out is None:
            out = dict(x=torch.empty((B, 4, T + 1), dtype=f, device=self.device),
                       u=torch.empty((B, 2, T), dtype=f, device=self.device),
                       status=torch.empty(B, dtype=torch.int32, device=self.device),
                       iters=torch.empty(B, dtype=torch.int32, device=self.device),
                       kkt=torch.empty((B, 4), dtype=f, device=self.device))
        self._chk(self.lib.mpcx_qp_solve_batch(self._ctx, B, _ptr(x0), _ptr(xref), _ptr(xbar), _ptr(reaches_end),
                                               _ptr(u_warm), _ptr(out['x']), _ptr(out['u']), _ptr(out['status']),
                                               _ptr(out['iters']), _ptr(out['kkt'])))
        return out

    @_ordered
    def prepare(self, state, u_warm, path, path_off, path_len, dl, target_ind, out=None, path_v=None, x_prev=None, stop_idx=None,
                v_ref=0.0, len_seen=None):
        """mpcx_mpc_prepare_batch. target_ind is updated in place. Returns dict(xref, reaches_end, xbar).
        x_prev (B, 4, T+1): the previous linearisation pass's states -- its speeds space the reference window (lib/mpc.py:226-237,
        MAX_ITER > 1; mpcx_mpc_prepare_batch_ov).
        stop_idx (B, int32): the stop index of lib/mpc_with_speed.py:276-282 over the WHOLE path (path_len = full lengths): xref[2] is
        v_ref (or path_v) in front of it and 0 from it on, _lib.NO_STOP = no stop; len_seen (B, int32, out) receives path_len
        (mpcx_mpc_prepare_batch_stop)."""
        T = self.params.T
        B = state.shape[0]
        f = torch.float64
        self._want(state, f, (B, 4), 'state'); self._want(path, f, None, 'path')
        self._want(path_off, torch.int32, (B,), 'path_off'); self._want(path_len, torch.int32, (B,), 'path_len')
        self._want(target_ind, torch.int32, (B,), 'target_ind')
        if u_warm is not None:
            self._want(u_warm, f, (B, 2, T), 'u_warm')
        if out is None:
            out = dict(xref=torch.empty((B, 4, T + 1), dtype=f, device=self.device),
                       reaches_end=torch.empty((B, T + 1), dtype=torch.uint8, device=self.device),
                       xbar=torch.empty((B, 4, T + 1), dtype=f, device=self.device))
        ov, stride = None, 0
        if x_prev is not None:
            self._want(x_prev, f, (B, 4, T + 1), 'x_prev')
            ov, stride = x_prev.data_ptr() + 2 * (T + 1) * 8, 4 * (T + 1)
        if stop_idx is not None:
            self._want(stop_idx, torch.int32, (B,), 'stop_idx')
            if len_seen is not None:
                self._want(len_seen, torch.int32, (B,), 'len_seen')
            self._chk(self.lib.mpcx_mpc_prepare_batch_stop(self._ctx, B, _ptr(state), _ptr(u_warm), _ptr(path), _ptr(path_v), _ptr(path_off),
                                                           _ptr(path_len), C.c_double(float(dl)), _ptr(target_ind), ov, stride,
                                                           _ptr(stop_idx), C.c_double(float(v_ref)), _ptr(len_seen),
                                                           _ptr(out['xref']), _ptr(out['reaches_end']), _ptr(out['xbar'])))
            return out
        self._chk(self.lib.mpcx_mpc_prepare_batch_ov(self._ctx, B, _ptr(state), _ptr(u_warm), _ptr(path), _ptr(path_v), _ptr(path_off),
                                                     _ptr(path_len), C.c_double(float(dl)), _ptr(target_ind), ov, stride,
                                                     _ptr(out['xref']), _ptr(out['reaches_end']), _ptr(out['xbar'])))
        return out

    @_ordered
    def plant_step(self, state, u, status, applied):
        B = state.shape[0]
        self._want(state, torch.float64, (B, 4), 'state'); self._want(applied, torch.float64, (B, 2), 'applied')
        self._chk(self.lib.mpcx_plant_step_batch(self._ctx, B, _ptr(state), _ptr(u), _ptr(status), _ptr(applied)))

    def search_model(self, templates, last_pose, edge_cost, hp, hp_off):
        return SearchModel(self, templates, last_pose, edge_cost, hp, hp_off)

    @_ordered
    def expand(self, model: 'SearchModel', nodes, out=None, nodes_cs=None):
        """mpcx_expand_batch: nodes (n,3) -> dict(nbr (n,P,3), cost (n,P), collide (n,P) uint8).
        nodes_cs (n,2): optional host-computed cos/sin of the headings (bit-exact replay of the reference's search)."""
        n = nodes.shape[0]
        self._want(nodes, torch.float64, (n, 3), 'nodes')
        if nodes_cs is not None:
            self._want(nodes_cs, torch.float64, (n, 2), 'nodes_cs')
        Pn = model.n_prim
        if out is None:
            out = dict(nbr=torch.empty((n, Pn, 3), dtype=torch.float64, device=self.device),
                       cost=torch.empty((n, Pn), dtype=torch.float64, device=self.device),
                       collide=torch.empty((n, Pn), dtype=torch.uint8, device=self.device))
        self._chk(self.lib.mpcx_expand_batch(self._ctx, model._h, n, _ptr(nodes), _ptr(nodes_cs), _ptr(out['nbr']), _ptr(out['cost']),
                                             _ptr(out['collide'])))
        return out

    @_ordered
    def astar_batch(self, models, specs, cs_theta, cs_val, ov_key=None, ov_val=None, max_expansions=4096, path_cap=64, heap_cap=None, push_cap=None):
        """mpcx_astar_batch: one device-resident best-first search per entry of `specs` (dicts: start, goal_box, goal_point,
        allowed_dtheta, variant [, wh, wc, hp_norm (device tensor), ov_off, ov_cnt]) against models[i]; cs_theta (ascending) / cs_val: the
        host's cos / sin table; ov_key (n, 4) / ov_val: the override table, every search's slice sorted as tuples.  Capacities: the log
        holds max_expansions expansions, the heap `heap_cap` entries and the successor log `push_cap` (default for both: what n_prim
        successors per expansion can need).  Returns a dict of device tensors: status, n_exp, n_push, cost, miss, path_len, path
        (n, path_cap, 3; goal first), path_prim, log (n, max_expansions, 8), push_log (n, push_cap, 8)."""
        n = len(specs)
        f, dev = torch.float64, self.device
        P = max(m.n_prim for m in models)
        full = max(16, P * max_expansions + 1)
        heap_cap = full if heap_cap is None else max(16, min(int(heap_cap), full))
        push_cap = full if push_cap is None else max(16, min(int(push_cap), full))
        table_cap = 1 << int(np.ceil(np.log2(2 * (max_expansions + 1))))
        # only the closed set needs a fill (NaN = empty slot); everything else is written by the kernel before anyone reads it
        out = dict(heap=torch.empty((n, heap_cap, 10), dtype=f, device=dev), table=torch.full((n, table_cap, 8), float('nan'), dtype=f, device=dev),
                   log=torch.empty((n, max_expansions, 8), dtype=f, device=dev), push_log=torch.empty((n, push_cap, 8), dtype=f, device=dev),
                   path=torch.empty((n, path_cap, 3), dtype=f, device=dev), path_prim=torch.empty((n, path_cap), dtype=torch.int32, device=dev),
                   cost=torch.empty(n, dtype=f, device=dev), miss=torch.zeros(n, dtype=f, device=dev),
                   status=torch.empty(n, dtype=torch.int32, device=dev), n_exp=torch.empty(n, dtype=torch.int32, device=dev),
                   n_push=torch.empty(n, dtype=torch.int32, device=dev), path_len=torch.empty(n, dtype=torch.int32, device=dev))
        b = _lib.AstarBuffersC()
        b.heap_cap, b.table_cap, b.log_cap, b.push_cap, b.path_cap = heap_cap, table_cap, max_expansions, push_cap, path_cap
        for k in ('heap', 'table', 'log', 'push_log', 'path', 'cost', 'miss', 'status', 'n_exp', 'n_push', 'path_len', 'path_prim'):
            setattr(b, k, out[k].data_ptr())
        if isinstance(specs, np.ndarray):       # rows of _lib.ASTAR_SEARCH_DTYPE, filled by the caller (hp_norm: device addresses it keeps alive)
            if specs.dtype != _lib.ASTAR_SEARCH_DTYPE:
                raise MpcxError('astar_batch: spec rows must have dtype _lib.ASTAR_SEARCH_DTYPE')
            rows = np.ascontiguousarray(specs)
        else:
            rows = np.zeros(n, dtype=_lib.ASTAR_SEARCH_DTYPE)
            for i, s in enumerate(specs):
                r = rows[i]
                r['start'] = s['start']; r['goal_box'] = s['goal_box']; r['goal_point'] = s['goal_point']
                r['allowed_dtheta'] = s['allowed_dtheta']
                r['wh'] = s.get('wh', (1.0, 2.7, 15.0, 0.0, 0.0)); r['wc'] = s.get('wc', (1.0, 5.0, 0.1, 0.0))
                hn = s.get('hp_norm')
                if hn is not None:
                    self._want(hn, f, (models[i].n_rows,), 'hp_norm')
                    r['hp_norm'] = hn.data_ptr()
                r['variant'] = s['variant']; r['ov_off'] = s.get('ov_off', 0); r['ov_cnt'] = s.get('ov_cnt', 0)
        rows['max_expansions'] = int(max_expansions)
        sp = C.c_void_p(rows.ctypes.data)
        hs = (C.c_void_p * n)(*[m._h for m in models])
        self._want(cs_theta, f, None, 'cs_theta'); self._want(cs_val, f, (cs_theta.shape[0], 2), 'cs_val')
        n_ov = 0 if ov_key is None else int(ov_key.shape[0])
        if n_ov:
            self._want(ov_key, f, (n_ov, 4), 'ov_key'); self._want(ov_val, f, (n_ov,), 'ov_val')
        self._chk(self.lib.mpcx_astar_batch(self._ctx, n, hs, sp, int(cs_theta.shape[0]), _ptr(cs_theta), _ptr(cs_val),
                                            n_ov, _ptr(ov_key) if n_ov else None, _ptr(ov_val) if n_ov else None, C.byref(b)))
        del out['heap'], out['table']
        return out

    @_ordered
    def expand_multi(self, models, seg_off, nodes, nodes_cs=None):
        """mpcx_expand_multi_batch: nodes (n,3) grouped by search, seg_off = n_seg+1 offsets (host ints), models = one
        SearchModel per segment.  Returns dict(nbr (n,P,3), cost (n,P), collide (n,P)) laid out like separate expand() calls."""
        n = nodes.shape[0]
        self._want(nodes, torch.float64, (n, 3), 'nodes')
        if nodes_cs is not None:
            self._want(nodes_cs, torch.float64, (n, 2), 'nodes_cs')
        Pn = models[0].n_prim
        out = dict(nbr=torch.empty((n, Pn, 3), dtype=torch.float64, device=self.device),
                   cost=torch.empty((n, Pn), dtype=torch.float64, device=self.device),
                   collide=torch.empty((n, Pn), dtype=torch.uint8, device=self.device))
        handles = (C.c_void_p * len(models))(*[m._h for m in models])
        offs = (C.c_int32 * (len(models) + 1))(*[int(v) for v in seg_off])
        self._chk(self.lib.mpcx_expand_multi_batch(self._ctx, len(models), handles, offs, _ptr(nodes), _ptr(nodes_cs), _ptr(out['nbr']),
                                                   _ptr(out['cost']), _ptr(out['collide'])))
        return out

    @_ordered
    def interaction(self, ip: InteractionParams, state, path, path_cs, path_off, path_len, prev_cut_len,
                    obs6, obs_off, obs_cnt, obs_skip, traj_idx, out=None, intent: Optional['_lib.IntentC'] = None, u_sol=None, status=None,
                    done=None, absent=None):
        """mpcx_interaction_batch. traj_idx updated in place. Returns dict(hit_idx, hit_xy, cut_len).
        intent: a _lib.IntentC -- mpcx_interaction_batch_intent: the shared-plans stage runs between the prediction and the conflict search
        on u_sol (P, 2, T float64) and status (P int32) of the previous solve; done (P int32) and absent (pool rows int32) are read by that
        stage alone and may be None."""
        Pn = state.shape[0]
        i32 = torch.int32
        self._want(state, torch.float64, (Pn, 4), 'state')
        self._want(path_cs, torch.float64, (path.shape[0], 2), 'path_cs')
        for nm, t in (('path_off', path_off), ('path_len', path_len), ('obs_off', obs_off), ('obs_cnt', obs_cnt), ('traj_idx', traj_idx)):
            self._want(t, i32, (Pn,), nm)
        if ip.path_cum is not None:
            self._want(ip.path_cum, torch.float64, (path.shape[0],), 'path_cum')
        if ip.path_first_within is not None:
            self._want(ip.path_first_within, torch.int32, (path.shape[0],), 'path_first_within')
        nobs = 0 if obs6 is None else obs6.shape[0]
        if out is None:
            out = dict(hit_idx=torch.empty(Pn, dtype=i32, device=self.device),
                       hit_xy=torch.empty((Pn, 2), dtype=torch.float64, device=self.device),
                       cut_len=torch.empty(Pn, dtype=i32, device=self.device))
        cip = ip.to_c()
        if intent is not None:
            if u_sol is None or status is None:
                raise MpcxError('interaction: intent needs u_sol and status (the previous solve)')
            self._want(u_sol, torch.float64, None if self.params is None else (Pn, 2, self.params.T), 'u_sol')
            self._want(status, i32, (Pn,), 'status')
            if done is not None:
                self._want(done, i32, (Pn,), 'done')
            if absent is not None:
                self._want(absent, i32, (nobs,), 'absent')
            self._chk(self.lib.mpcx_interaction_batch_intent(self._ctx, C.byref(cip), Pn, _ptr(state), _ptr(path), _ptr(path_cs),
                                                             _ptr(path_off), _ptr(path_len), _ptr(prev_cut_len), nobs, _ptr(obs6),
                                                             _ptr(obs_off), _ptr(obs_cnt), _ptr(obs_skip), _ptr(traj_idx),
                                                             _ptr(out['hit_idx']), _ptr(out['hit_xy']), _ptr(out['cut_len']),
                                                             _ptr(u_sol), _ptr(status), _ptr(done), _ptr(absent), C.byref(intent)))
            return out
        self._chk(self.lib.mpcx_interaction_batch(self._ctx, C.byref(cip), Pn, _ptr(state), _ptr(path), _ptr(path_cs),
                                                  _ptr(path_off), _ptr(path_len), _ptr(prev_cut_len), nobs, _ptr(obs6),
                                                  _ptr(obs_off), _ptr(obs_cnt), _ptr(obs_skip), _ptr(traj_idx),
                                                  _ptr(out['hit_idx']), _ptr(out['hit_xy']), _ptr(out['cut_len'])))
        return out

    @_ordered
    def moving_collision(self, ip: InteractionParams, ego, ego_cs, ego_off, ego_len, path, path_cs, path_off, path_len,
                         obs, obs_cs, obs_off, obs_cnt, out=None):
        """mpcx_moving_collision_batch (explicit trajectories). Returns dict(hit_idx, hit_xy).
        obs / obs_cs: the obstacle trajectories, ip.pred_steps poses each, as (n, pred_steps, 3) / (n, pred_steps, 2) or with the first two
        axes flattened; obs_off / obs_cnt count TRAJECTORIES.  The pool size handed to the library is the number of trajectories: it
        reads pred_steps poses per pool entry, so the number of rows of a flattened table would send it pred_steps times past the end."""
        Pn = ego_off.shape[0]
        if out is None:
            out = dict(hit_idx=torch.empty(Pn, dtype=torch.int32, device=self.device),
                       hit_xy=torch.empty((Pn, 2), dtype=torch.float64, device=self.device))
        nobs = 0
        if obs is not None:
            steps = int(ip.pred_steps)
            if steps < 1 or obs.dtype != torch.float64 or obs.numel() % (3 * steps) or not obs.is_contiguous():
                raise MpcxError('moving_collision: obs must be a contiguous float64 table of whole trajectories of pred_steps = %d poses '
                                '(x, y, yaw), got shape %s' % (steps, tuple(obs.shape)))
            nobs = obs.numel() // (3 * steps)
            self._want(obs_cs, torch.float64, None, 'obs_cs')
            if obs_cs.numel() != 2 * nobs * steps:
                raise MpcxError('moving_collision: obs_cs must hold cos / sin of every pose of obs (%d x %d x 2), got shape %s'
                                % (nobs, steps, tuple(obs_cs.shape)))
        cip = ip.to_c()
        self._chk(self.lib.mpcx_moving_collision_batch(self._ctx, C.byref(cip), Pn, _ptr(ego), _ptr(ego_cs), _ptr(ego_off),
                                                       _ptr(ego_len), _ptr(path), _ptr(path_cs), _ptr(path_off), _ptr(path_len),
                                                       nobs, _ptr(obs), _ptr(obs_cs), _ptr(obs_off), _ptr(obs_cnt),
                                                       _ptr(out['hit_idx']), _ptr(out['hit_xy'])))
        return out

    @_ordered
    def transform(self, nodes, pts_off, pts_cnt, pts, max_pts):
        """mpcx_transform_batch -> (n, max_pts, 3)"""
        n = nodes.shape[0]
        out = torch.empty((n, max_pts, 3), dtype=torch.float64, device=self.device)
        self._chk(self.lib.mpcx_transform_batch(self._ctx, n, int(max_pts), _ptr(nodes), _ptr(pts_off), _ptr(pts_cnt), _ptr(pts), _ptr(out)))
        return out

    @_ordered
    def cutoff_index(self, pts, off, ln, xy, radius=0.001):
        Pn = off.shape[0]
        out = torch.empty(Pn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.mpcx_cutoff_index_batch(self._ctx, Pn, _ptr(pts), _ptr(off), _ptr(ln), _ptr(xy), C.c_double(radius), _ptr(out)))
        return out

    @_ordered
    def predict_obstacles(self, obs6, steps, dt, L):
        n = obs6.shape[0]
        out = torch.empty((n, steps, 3), dtype=torch.float64, device=self.device)
        self._chk(self.lib.mpcx_predict_obstacles_batch(self._ctx, n, int(steps), C.c_double(dt), C.c_double(L), _ptr(obs6), _ptr(out)))
        return out

    @_ordered
    def traffic_step(self, actors, actor_state, pool_row, obs6, tape=None):
        """mpcx_traffic_step_batch: every scripted actor writes its get() row (x, y, v, yaw, a, steer) into row pool_row[i] of obs6 and
        takes its step().  actors: uint8 device tensor holding n records of _lib.TRAFFIC_ACTOR_DTYPE; actor_state (n, 4) float64, updated in
        place; tape (rows, 6) float64 or None."""
        n = int(actor_state.shape[0])
        self._want(actors, torch.uint8, (n * _lib.TRAFFIC_ACTOR_DTYPE.itemsize,), 'actors')
        self._want(actor_state, torch.float64, (n, 4), 'actor_state'); self._want(pool_row, torch.int32, (n,), 'pool_row')
        self._want(obs6, torch.float64, (obs6.shape[0], 6), 'obs6')
        if tape is not None:
            self._want(tape, torch.float64, (tape.shape[0], 6), 'tape')
        self._chk(self.lib.mpcx_traffic_step_batch(self._ctx, n, _ptr(actors), _ptr(actor_state), _ptr(tape), 0 if tape is None else int(tape.shape[0]),
                                                   _ptr(pool_row), int(obs6.shape[0]), _ptr(obs6)))

    @_ordered
    def closed_loop_run(self, ip: InteractionParams, desc: '_lib.ClosedLoopC', n_steps: int, graph: bool = False, **stages):
        """mpcx_closed_loop_run: n_steps of the scenario loop body on the buffers `desc` names, no host work between.
        **stages: one keyword per optional stage, the stage's struct or None = off.  _lib.STAGES lists them, each with what it does, what
        it is refused without and what None means; a keyword that is not in that list is a TypeError."""
        structs = _lib.stage_structs(stages)
        # (the widest entry point: NULL is "none" for every stage, and the narrower ones are that call with NULLs)
        run = getattr(self.lib, _lib.LOOP_ENTRY_POINTS[-1])
        self._chk(run(self._ctx, C.byref(ip.to_c()), C.byref(desc), *(None if s is None else C.byref(s) for s in structs), int(n_steps),
                      1 if graph else 0))

    @_ordered
    def signal_step(self, dl: float, state, path_off, path_len, traj_idx, cut_len, signals: '_lib.SignalsC', done=None):
        """mpcx_signal_step_batch: ONE step's signal stage as the closed loop enqueues it between the conflict search and the window stage.
        cut_len (P int32: the conflict search's cut length, or stop index in speed mode) is updated in place, as are the struct's tick and
        held; done: the retirement words (P int32) or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_signal_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                  _ptr(cut_len), _ptr(done), C.byref(signals)))

    @_ordered
    def actuated_step(self, dl: float, state, path_off, path_len, traj_idx, cut_len, signals: '_lib.SignalsC', actuation: '_lib.ActuationC',
                      done=None):
        """mpcx_actuated_step_batch: ONE step's actuated signal stage as the closed loop enqueues it in the place of the signal stage.
        cut_len (P int32) is updated in place, as are the signals' held and the controller's jstate, lights and calls; done: the retirement
        words (P int32) or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_actuated_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                    _ptr(cut_len), _ptr(done), C.byref(signals), C.byref(actuation)))

    @_ordered
    def reserve_step(self, dl: float, state, path_off, path_len, traj_idx, cut_len, signals: '_lib.SignalsC', reservation: '_lib.ReservationC',
                     done=None):
        """mpcx_reserve_step_batch: ONE step's reservation stage as the closed loop enqueues it in the place of the signal stage.
        cut_len (P int32) is updated in place, as are the signals' held and the reservation's grant, since, clock, occupied and queued; done:
        the retirement words (P int32) or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_reserve_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                   _ptr(cut_len), _ptr(done), C.byref(signals), C.byref(reservation)))

    @_ordered
    def advise_step(self, dl: float, path_off, path_len, traj_idx, cut_len, signals: '_lib.SignalsC', advice: '_lib.AdviceC', xref, done=None):
        """mpcx_advise_step_batch: ONE step's advice stage as the closed loop enqueues it between the window stage and the QP, in speed mode.
        xref (P, 4, T + 1 float64: the window stage's output of this step) has row 2 of every advised agent capped in place, and the
        struct's advised is written; traj_idx and cut_len (P int32) as the signal stage left them; done: the retirement words or None."""
        if self.params is None:
            raise MpcxError('advise_step: set_mpc_params has not been called (the stage sizes the window from the horizon)')
        Pn = int(xref.shape[0])
        self._want(xref, torch.float64, (Pn, 4, self.params.T + 1), 'xref')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_advise_step_batch(self._ctx, Pn, float(dl), _ptr(path_off), _ptr(path_len), _ptr(traj_idx), _ptr(cut_len),
                                                  _ptr(done), C.byref(signals), C.byref(advice), _ptr(xref)))

    @_ordered
    def admit_step(self, ip: InteractionParams, state, obs_off, obs_cnt, obs_skip, done, absent, admit: '_lib.AdmitC', actors=None,
                   actor_state=None, actor_row=None, tape=None, precedence: Optional['_lib.PrecedenceC'] = None):
        """mpcx_admit_step_batch: ONE step's admission as the closed loop enqueues it at the head of a step.  done (P) and absent (pool
        rows) are the retirement and scene words, int32, updated in place; admit: a _lib.AdmitC naming caller-owned device buffers (wait and
        entered_step: P int32, clock: 1 int32).  actors / actor_state / actor_row / tape: scripted cars as traffic_step takes them; they
        are read, not stepped.
        precedence: a _lib.PrecedenceC -- mpcx_admit_step_batch_precedence: in ENTRY mode the entry-order stamp follows the admission, as
        at the head of a closed-loop step with right of way."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state'); self._want(done, torch.int32, (Pn,), 'done')
        self._want(absent, torch.int32, (absent.shape[0],), 'absent')
        for nm, t in (('obs_off', obs_off), ('obs_cnt', obs_cnt), ('obs_skip', obs_skip)):
            self._want(t, torch.int32, (Pn,), nm)
        n = 0
        if actor_state is not None:
            n = int(actor_state.shape[0])
            self._want(actors, torch.uint8, (n * _lib.TRAFFIC_ACTOR_DTYPE.itemsize,), 'actors')
            self._want(actor_state, torch.float64, (n, 4), 'actor_state'); self._want(actor_row, torch.int32, (n,), 'actor_row')
            if tape is not None:
                self._want(tape, torch.float64, (tape.shape[0], 6), 'tape')
        cip = ip.to_c()
        args = (self._ctx, C.byref(cip), Pn, _ptr(state), _ptr(obs_off), _ptr(obs_cnt), _ptr(obs_skip), _ptr(done),
                int(absent.shape[0]), _ptr(absent), n, _ptr(actors) if n else None,
                _ptr(actor_state) if n else None, _ptr(tape) if n else None,
                0 if (tape is None or not n) else int(tape.shape[0]), _ptr(actor_row) if n else None,
                C.byref(admit))
        if precedence is not None:
            self._chk(self.lib.mpcx_admit_step_batch_precedence(*args, C.byref(precedence)))
            return
        self._chk(self.lib.mpcx_admit_step_batch(*args))

    @_ordered
    def respawn_step(self, state, applied, u_sol, traj_idx, target_ind, cut_len, iters, obs_skip, n_obs_pool: int, retire: '_lib.RetireC',
                     admit: '_lib.AdmitC', respawn: '_lib.RespawnC', prev_len=None, log: Optional['_lib.RunLogC'] = None,
                     routes: Optional['_lib.RoutesC'] = None, max_path_len: int = 0):
        """mpcx_respawn_step_batch: ONE step's respawn as the closed loop enqueues it at the end of a step (after the retire stage).  The
        buffers are the closed loop's, updated in place: state (P, 4), applied (P, 2), u_sol (P, 2, T), int32 traj_idx, target_ind, cut_len,
        iters (P each), prev_len (P; the speed stop mode only); obs_skip names the agents' own rows among the n_obs_pool rows of the pool.
        retire / admit / respawn / log: structs naming caller-owned device buffers (done is read, steps_driven, wait, entered_step, served,
        the episode table and the log's outcome words are written).
        routes: a _lib.RoutesC -- mpcx_respawn_step_batch_routes: the reset also writes the next vehicle's route (routes.path_off / path_len,
        P int32 each), start pose and index; max_path_len bounds the route lengths (0: no upper bound)."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state'); self._want(applied, torch.float64, (Pn, 2), 'applied')
        self._want(u_sol, torch.float64, (Pn, 2, self.params.T), 'u_sol')
        for nm, t in (('traj_idx', traj_idx), ('target_ind', target_ind), ('cut_len', cut_len), ('iters', iters), ('obs_skip', obs_skip)):
            self._want(t, torch.int32, (Pn,), nm)
        if prev_len is not None:
            self._want(prev_len, torch.int32, (Pn,), 'prev_len')
        if routes is not None:
            self._chk(self.lib.mpcx_respawn_step_batch_routes(self._ctx, Pn, _ptr(state), _ptr(applied), _ptr(u_sol), _ptr(traj_idx),
                                                              _ptr(target_ind), _ptr(cut_len), _ptr(iters), _ptr(prev_len), _ptr(obs_skip),
                                                              int(n_obs_pool), None if log is None else C.byref(log), C.byref(retire),
                                                              C.byref(admit), C.byref(respawn), C.byref(routes), int(max_path_len)))
            return
        self._chk(self.lib.mpcx_respawn_step_batch(self._ctx, Pn, _ptr(state), _ptr(applied), _ptr(u_sol), _ptr(traj_idx), _ptr(target_ind),
                                                   _ptr(cut_len), _ptr(iters), _ptr(prev_len), _ptr(obs_skip), int(n_obs_pool),
                                                   None if log is None else C.byref(log), C.byref(retire), C.byref(admit), C.byref(respawn)))

    @_ordered
    def episode_summary(self, A: int, R: int, served, ep_i32, ep_f64):
        """mpcx_episode_summary: the per-instance, per-route table of the finished episodes of a routed run, reduced on the device.
        served (P,), ep_i32 (P, G, 8) int32, ep_f64 (P, G, 2) float64, P = B A.  Returns device tensors (B, R, 4) int64 -- _lib.SUMMARY_I64:
        count, contacts, sum of entered - due, sum of steps_driven -- and (B, R) float64, the minimum of min_clearance (+inf: none)."""
        Pn, G = int(ep_i32.shape[0]), int(ep_i32.shape[1])
        self._want(served, torch.int32, (Pn,), 'served'); self._want(ep_i32, torch.int32, (Pn, G, 8), 'ep_i32')
        self._want(ep_f64, torch.float64, (Pn, G, 2), 'ep_f64')
        if A < 1 or Pn % int(A):
            raise MpcxError('episode_summary: %d slots do not divide into instances of %d (MPCX_E_INVALID)' % (Pn, A))
        B = Pn // int(A)
        out_i = torch.zeros((B, int(R), 4), dtype=torch.int64, device=self.device)
        out_f = torch.full((B, int(R)), float('inf'), dtype=torch.float64, device=self.device)
        self._chk(self.lib.mpcx_episode_summary(self._ctx, Pn, int(A), G, int(R), _ptr(served), _ptr(ep_i32), _ptr(ep_f64), _ptr(out_i), _ptr(out_f)))
        return out_i, out_f

    @_ordered
    def record_step(self, ip: InteractionParams, state, applied, x_sol, path, path_off, path_len, target_ind, cut_len, traj_idx, hit_idx,
                    status, iters, obs6, obs_off, obs_cnt, obs_skip, log: '_lib.RunLogC', goal_len=None):
        """mpcx_record_step_batch: the run log's record of ONE step, from the closed loop's buffers as the plant step leaves them
        (obs6: the pool as the step's conflict search saw it).  log: a _lib.RunLogC naming caller-owned device buffers.
        goal_len (P, int32): len(self.cx) of the goal test instead of cut_len (mpcx_record_step_batch_goal)."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state'); self._want(applied, torch.float64, (Pn, 2), 'applied')
        self._want(x_sol, torch.float64, (Pn, 4, self.params.T + 1), 'x_sol'); self._want(obs6, torch.float64, (obs6.shape[0], 6), 'obs6')
        for nm, t in (('path_off', path_off), ('path_len', path_len), ('target_ind', target_ind), ('cut_len', cut_len), ('traj_idx', traj_idx),
                      ('hit_idx', hit_idx), ('status', status), ('iters', iters), ('obs_off', obs_off), ('obs_cnt', obs_cnt)):
            self._want(t, torch.int32, (Pn,), nm)
        if obs_skip is not None:
            self._want(obs_skip, torch.int32, (Pn,), 'obs_skip')
        cip = ip.to_c()
        if goal_len is not None:
            self._want(goal_len, torch.int32, (Pn,), 'goal_len')
            self._chk(self.lib.mpcx_record_step_batch_goal(self._ctx, C.byref(cip), Pn, _ptr(state), _ptr(applied), _ptr(x_sol), _ptr(path),
                                                           _ptr(path_off), _ptr(path_len), _ptr(target_ind), _ptr(cut_len), _ptr(traj_idx),
                                                           _ptr(hit_idx), _ptr(status), _ptr(iters), int(obs6.shape[0]), _ptr(obs6), _ptr(obs_off),
                                                           _ptr(obs_cnt), _ptr(obs_skip), _ptr(goal_len), C.byref(log)))
            return
        self._chk(self.lib.mpcx_record_step_batch(self._ctx, C.byref(cip), Pn, _ptr(state), _ptr(applied), _ptr(x_sol), _ptr(path), _ptr(path_off),
                                                  _ptr(path_len), _ptr(target_ind), _ptr(cut_len), _ptr(traj_idx), _ptr(hit_idx), _ptr(status),
                                                  _ptr(iters), int(obs6.shape[0]), _ptr(obs6), _ptr(obs_off), _ptr(obs_cnt), _ptr(obs_skip),
                                                  C.byref(log)))

    @_ordered
    def closed_loop_stats(self, reset: bool = True):
        """mpcx_closed_loop_stats: dict(agent_steps, iterations, failures, max_iterations) accumulated on the device by
        closed_loop_run since the last reset (synchronises)"""
        out = (C.c_int64 * 4)()
        self._chk(self.lib.mpcx_closed_loop_stats(self._ctx, out, 1 if reset else 0))
        return dict(agent_steps=int(out[0]), iterations=int(out[1]), failures=int(out[2]), max_iterations=int(out[3]))

    def closed_loop_queue(self, P: int):
        """mpcx_closed_loop_queue: (order, keyslot), int32 host arrays of P words -- the QP work queue as the last closed-loop step left
        it and the (key << 24 | slot) every agent was filed under (synchronises)"""
        order, keyslot = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        self._chk(self.lib.mpcx_closed_loop_queue(self._ctx, int(P), order.ctypes.data, keyslot.ctypes.data))
        return order, keyslot

    def interaction_prediction(self, rows: int, steps: int):
        """mpcx_interaction_prediction: the obstacle prediction of the last interaction() / closed-loop step, float64 host array
        (rows, steps, 2, 2) of disc centres (synchronises)"""
        out = np.zeros((int(rows), int(steps), 2, 2))
        self._chk(self.lib.mpcx_interaction_prediction(self._ctx, int(rows), int(steps), out.ctypes.data))
        return out

    @_ordered
    def set_instance_tuning(self, rows: Optional[torch.Tensor]):
        """mpcx_set_instance_tuning: rows (B,16) float64 device tensor (MpcParams.tuning_row per problem) or None to clear.
        The tensor is kept alive by the context while set."""
        if rows is None:
            self._chk(self.lib.mpcx_set_instance_tuning(self._ctx, None, 0))
        else:
            self._want(rows, torch.float64, (rows.shape[0], 16), 'tuning rows')
            self._chk(self.lib.mpcx_set_instance_tuning(self._ctx, _ptr(rows), int(rows.shape[0])))
        self._tuning = rows

    def set_following(self, following: Optional['_lib.FollowingC']):
        """mpcx_set_following: car following for every closed-loop run of this context from now on; None (or an all-zero struct) = off.
        The context copies the struct; the device buffers it names (leader, gap, cap) stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_following(self._ctx, None if following is None else C.byref(following)))
        self._following = following

    def set_safety(self, safety: Optional['_lib.SafetyC']):
        """mpcx_set_safety: the near-miss log for every closed-loop run of this context from now on; None (or an all-zero struct) = off.
        The context copies the struct; the device buffers it names stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_safety(self._ctx, None if safety is None else C.byref(safety)))
        self._safety = safety

    def set_sight(self, sight: Optional['_lib.SightC']):
        """mpcx_set_sight: line of sight for every closed-loop run of this context from now on; None (or an all-zero struct) = off.  The
        context copies the struct; the device buffers it names stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_sight(self._ctx, None if sight is None else C.byref(sight)))
        self._sight = sight

    def set_keepclear(self, keepclear: Optional['_lib.KeepClearC']):
        """mpcx_set_keepclear: keep clear for every closed-loop run of this context from now on; None (or an all-zero struct) = off.  The
        context copies the struct; the device buffers it names stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_keepclear(self._ctx, None if keepclear is None else C.byref(keepclear)))
        self._keepclear = keepclear

    @_ordered
    def keepclear_step(self, dl: float, state, path_off, path_len, traj_idx, cut_len, signals: '_lib.SignalsC', keepclear: '_lib.KeepClearC',
                       done=None):
        """mpcx_keepclear_step_batch: ONE step's keep-clear stage as the closed loop enqueues it behind the signal / actuated stage, on the
        signals' held as that stage left it.  cut_len (P int32) is lowered in place for a boxed agent, and the struct's boxed, waited,
        occupied and n_boxed are written; done: the retirement words (P int32) or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_keepclear_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                     _ptr(cut_len), _ptr(done), None if signals is None else C.byref(signals),
                                                     C.byref(keepclear)))

    def set_priority(self, priority: Optional['_lib.PriorityC']):
        """mpcx_set_priority: the priority rule for every closed-loop run of this context from now on; None (or an all-zero struct) = off.
        The context copies the struct; the device buffers it names stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_priority(self._ctx, None if priority is None else C.byref(priority)))
        self._priority = priority

    @_ordered
    def priority_step(self, dl: float, state, path_off, path_len, traj_idx, cut_len, priority: '_lib.PriorityC', done=None):
        """mpcx_priority_step_batch: ONE step's priority stage as the closed loop enqueues it in the hold's place.  cut_len (P int32) is
        lowered in place for a yielding agent, and the struct's waited, yielding, blocker, lag, occupied and n_yielding are written; done:
        the retirement words (P int32) or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_priority_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                    _ptr(cut_len), _ptr(done), C.byref(priority)))

    def set_stopsign(self, stopsign: Optional['_lib.StopSignC']):
        """mpcx_set_stopsign: the stop-sign rule for every closed-loop run of this context from now on; None (or an all-zero struct) = off.
        The context copies the struct; the device buffers it names stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_stopsign(self._ctx, None if stopsign is None else C.byref(stopsign)))
        self._stopsign = stopsign

    @_ordered
    def stopsign_step(self, dl: float, state, path_off, path_len, traj_idx, cut_len, stopsign: '_lib.StopSignC', done=None):
        """mpcx_stopsign_step_batch: ONE step's stop-sign stage as the closed loop enqueues it in the hold's place.  cut_len (P int32) is
        lowered in place for an agent held at its line, and the struct's stopped_at, go, stopping, clock, ran, lag, blocker, occupied and
        n_waiting are written; done: the retirement words (P int32) or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len)):
            self._want(t, torch.int32, (Pn,), name)
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_stopsign_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                    _ptr(cut_len), _ptr(done), C.byref(stopsign)))

    def set_braking(self, braking: Optional['_lib.BrakingC']):
        """mpcx_set_braking: the firm hold for every closed-loop run of this context from now on; None (or an all-zero struct) = off.  The
        context copies the struct; the device buffers it names stay the caller's and are kept alive here while set."""
        self._chk(self.lib.mpcx_set_braking(self._ctx, None if braking is None else C.byref(braking)))
        self._braking = braking

    @_ordered
    def brake_mark_step(self, dl: float, stop_mode: int, path_off, path_len, traj_idx, target_ind, win_len, path_stop, braking: '_lib.BrakingC',
                        held=None, boxed=None, yielding=None, done=None):
        """mpcx_brake_mark_step_batch: ONE step's firm-hold mark as the closed loop enqueues it in front of the window stage.  The struct's
        firm and brake_cap are written; in speed mode target_ind (P int32) is clamped in place and win_len (P int32) receives the lengths the
        window stage is to be handed in place of path_len.  path_stop: the stop-line table (n_points int32); held, boxed, yielding: the hold
        words that are on (P int32 each or None); done: the retirement words or None."""
        Pn = int(path_off.shape[0])
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('target_ind', target_ind), ('win_len', win_len),
                        ('held', held), ('boxed', boxed), ('yielding', yielding), ('done', done)):
            if t is not None:
                self._want(t, torch.int32, (Pn,), name)
        n_points = 0 if path_stop is None else int(path_stop.shape[0])
        if path_stop is not None:
            self._want(path_stop, torch.int32, (n_points,), 'path_stop')
        self._chk(self.lib.mpcx_brake_mark_step_batch(self._ctx, Pn, float(dl), int(stop_mode), _ptr(path_off), _ptr(path_len), _ptr(traj_idx),
                                                      _ptr(target_ind), _ptr(win_len), _ptr(done), _ptr(path_stop), n_points, _ptr(held), _ptr(boxed),
                                                      _ptr(yielding), C.byref(braking)))

    @_ordered
    def brake_clamp_step(self, dl: float, state, path, path_off, path_len, traj_idx, path_stop, braking: '_lib.BrakingC', xref, prev_len=None,
                         done=None):
        """mpcx_brake_clamp_step_batch: ONE step's firm-hold clamp as the closed loop enqueues it behind a window stage in speed mode: for
        every agent the mark left a stop index for, row 2 of xref (P, 4, T + 1 float64) is capped in place by the braking profile, traj_idx is
        pinned while the agent is behind its line, the struct's overran and brake_cap are written and prev_len (P int32 or None) is restored
        to the whole path's length."""
        if self.params is None:
            raise MpcxError('brake_clamp_step: set_mpc_params has not been called (the stage sizes the window from the horizon)')
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state')
        self._want(xref, torch.float64, (Pn, 4, self.params.T + 1), 'xref')
        self._want(path, torch.float64, (int(path.shape[0]), 3), 'path')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('prev_len', prev_len), ('done', done)):
            if t is not None:
                self._want(t, torch.int32, (Pn,), name)
        n_points = 0 if path_stop is None else int(path_stop.shape[0])
        if path_stop is not None:
            self._want(path_stop, torch.int32, (n_points,), 'path_stop')
        self._chk(self.lib.mpcx_brake_clamp_step_batch(self._ctx, Pn, float(dl), _ptr(state), _ptr(path), _ptr(path_off), _ptr(path_len),
                                                       _ptr(traj_idx), _ptr(prev_len), _ptr(done), _ptr(path_stop), n_points, C.byref(braking),
                                                       _ptr(xref)))

    @_ordered
    def sight_step(self, state, obs6, obs_off, obs_cnt, obs_skip, sight: '_lib.SightC', done=None, absent=None):
        """mpcx_sight_step_batch: ONE step's sight stage as the closed loop enqueues it in front of the conflict search: the struct's sight,
        n_seen and n_hidden words are written.  state (P, 4); obs6 (pool rows, 6): the pool as the head of the step packed it; done: the
        retirement words (P int32), absent: the scene's words (pool rows), or None."""
        Pn, rows = int(state.shape[0]), int(obs6.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state'); self._want(obs6, torch.float64, (rows, 6), 'obs6')
        for name, t in (('obs_off', obs_off), ('obs_cnt', obs_cnt), ('obs_skip', obs_skip), ('done', done)):
            if t is not None:
                self._want(t, torch.int32, (Pn,), name)
        if absent is not None:
            self._want(absent, torch.int32, (rows,), 'absent')
        self._chk(self.lib.mpcx_sight_step_batch(self._ctx, Pn, _ptr(state), _ptr(done), rows, _ptr(obs6), _ptr(obs_off), _ptr(obs_cnt),
                                                 _ptr(obs_skip), _ptr(absent), C.byref(sight)))

    @_ordered
    def safety_step(self, ip: InteractionParams, state, path_off, traj_idx, obs6, obs_off, obs_cnt, obs_skip, safety: '_lib.SafetyC', pred=None,
                    done=None, absent=None):
        """mpcx_safety_step_batch: ONE step's safety stage as the closed loop enqueues it behind the conflict search: the struct's per-step
        words, encounter words and event records are written.  obs6 (pool rows, 6): the pool as the head of the step packed it; pred
        (pool rows, ip.pred_steps, 2, 2) float64: the predicted disc centres, None = the context's own prediction as its last conflict
        search (interaction() or a closed-loop step) left it; done: the retirement words (P int32), absent: the scene's words (pool rows),
        or None."""
        Pn, rows = int(state.shape[0]), int(obs6.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state'); self._want(obs6, torch.float64, (rows, 6), 'obs6')
        for name, t in (('path_off', path_off), ('traj_idx', traj_idx), ('obs_off', obs_off), ('obs_cnt', obs_cnt), ('obs_skip', obs_skip),
                        ('done', done)):
            if t is not None:
                self._want(t, torch.int32, (Pn,), name)
        if absent is not None:
            self._want(absent, torch.int32, (rows,), 'absent')
        if pred is not None:
            self._want(pred, torch.float64, (rows, int(ip.pred_steps), 2, 2), 'pred')
        cip = ip.to_c()
        self._chk(self.lib.mpcx_safety_step_batch(self._ctx, C.byref(cip), Pn, _ptr(state), _ptr(path_off), _ptr(traj_idx), _ptr(done), rows,
                                                  _ptr(obs6), _ptr(pred), _ptr(obs_off), _ptr(obs_cnt), _ptr(obs_skip), _ptr(absent),
                                                  C.byref(safety)))

    @_ordered
    def safety_summary(self, A: int, route_off, dt: float, n_events, ev_i32, ev_f64):
        """mpcx_safety_summary: the conflict matrix of the near-miss log per instance of A consecutive agents and pair of movements, reduced
        on the device.  route_off (R,) int32: the routes' offsets into the path tables (an event side whose path_off word is none of them
        is class R: an actor, or an unknown offset); n_events (P,), ev_i32 (P, capacity, 8) int32, ev_f64 (P, capacity, 2) float64, P = B A.
        Returns device tensors (B, R + 1, R + 1, 3) int64 -- _lib.SAFETY_SUMMARY_I64: events, events with a contact, events with a predicted
        contact -- and (B, R + 1, R + 1, 2) float64 -- the minimum clearance and the shortest time to a predicted contact (s); +inf: none."""
        Pn, cap = int(ev_i32.shape[0]), int(ev_i32.shape[1])
        R = 0 if route_off is None else int(route_off.shape[0])
        self._want(n_events, torch.int32, (Pn,), 'n_events'); self._want(ev_i32, torch.int32, (Pn, cap, 8), 'ev_i32')
        self._want(ev_f64, torch.float64, (Pn, cap, 2), 'ev_f64')
        if route_off is not None:
            self._want(route_off, torch.int32, (R,), 'route_off')
        if A < 1 or Pn % int(A):
            raise MpcxError('safety_summary: %d agents do not divide into instances of %d (MPCX_E_INVALID)' % (Pn, A))
        B = Pn // int(A)
        out_i = torch.zeros((B, R + 1, R + 1, 3), dtype=torch.int64, device=self.device)
        out_f = torch.full((B, R + 1, R + 1, 2), float('inf'), dtype=torch.float64, device=self.device)
        self._chk(self.lib.mpcx_safety_summary(self._ctx, Pn, int(A), cap, R, _ptr(route_off), float(dt), _ptr(n_events), _ptr(ev_i32),
                                               _ptr(ev_f64), _ptr(out_i), _ptr(out_f)))
        return out_i, out_f

    @_ordered
    def follow_step(self, dl: float, stop_mode: int, state, path, path_off, path_len, traj_idx, cut_len, obs6, obs_off, obs_cnt,
                    following: '_lib.FollowingC', obs_skip=None, done=None, absent=None):
        """mpcx_follow_step_batch: ONE step's following search as the closed loop enqueues it in front of the window stage.  cut_len (P int32:
        the cut length, or stop index in speed mode) is lowered in place and the struct's leader, gap and cap are written; stop_mode:
        _lib.STOP_CUT or _lib.STOP_SPEED; obs6 (pool rows, 6): the pool as the head of the step packed it; obs_skip: the agents' own rows,
        done: the retirement words (P int32 each), absent: the scene's words (pool rows), or None."""
        Pn = int(state.shape[0])
        self._want(state, torch.float64, (Pn, 4), 'state'); self._want(obs6, torch.float64, (obs6.shape[0], 6), 'obs6')
        self._want(path, torch.float64, (path.shape[0], 3), 'path')
        for name, t in (('path_off', path_off), ('path_len', path_len), ('traj_idx', traj_idx), ('cut_len', cut_len), ('obs_off', obs_off),
                        ('obs_cnt', obs_cnt), ('obs_skip', obs_skip), ('done', done)):
            if t is not None:
                self._want(t, torch.int32, (Pn,), name)
        if absent is not None:
            self._want(absent, torch.int32, (obs6.shape[0],), 'absent')
        self._chk(self.lib.mpcx_follow_step_batch(self._ctx, Pn, float(dl), int(stop_mode), _ptr(state), _ptr(path), _ptr(path_off), _ptr(path_len),
                                                  _ptr(traj_idx), _ptr(cut_len), _ptr(done), int(obs6.shape[0]), _ptr(obs6), _ptr(obs_off),
                                                  _ptr(obs_cnt), _ptr(obs_skip), _ptr(absent), C.byref(following)))

    @_ordered
    def follow_cap_step(self, following: '_lib.FollowingC', xref, done=None):
        """mpcx_follow_cap_step_batch: ONE step's following clamp as the closed loop enqueues it behind a window stage in speed mode: row 2 of
        xref (P, 4, T + 1 float64) is capped in place at the struct's cap, as follow_step left it, for every agent with a leader."""
        if self.params is None:
            raise MpcxError('follow_cap_step: set_mpc_params has not been called (the stage sizes the window from the horizon)')
        Pn = int(xref.shape[0])
        self._want(xref, torch.float64, (Pn, 4, self.params.T + 1), 'xref')
        if done is not None:
            self._want(done, torch.int32, (Pn,), 'done')
        self._chk(self.lib.mpcx_follow_cap_step_batch(self._ctx, Pn, _ptr(done), C.byref(following), _ptr(xref)))

    @_ordered
    def set_qp_order_hint(self, prev_iters: Optional[torch.Tensor], ref_now: Optional[torch.Tensor] = None,
                          ref_prev: Optional[torch.Tensor] = None):
        """mpcx_qp_set_order_hint: int32 device tensors -- the previous solve's iteration counts (may be the `iters` output) and,
        optionally, a pair whose inequality marks problems whose reference jumped (e.g. cut lengths now / before); None clears"""
        for t in (prev_iters, ref_now, ref_prev):
            if t is not None:
                self._want(t, torch.int32, None, 'order hint')
        self._chk(self.lib.mpcx_qp_set_order_hint(self._ctx, _ptr(prev_iters), _ptr(ref_now), _ptr(ref_prev)))
        self._order_hint = (prev_iters, ref_now, ref_prev)

    def set_qp_solver(self, which: str):
        """'auto', 'condensed' (one wavefront per QP) or 'stage' (stage-structured solver, eight lanes per QP)"""
        self._chk(self.lib.mpcx_set_qp_solver(self._ctx, {'auto': 0, 'condensed': 1, 'stage': 2}[which]))

    def set_linearisation_passes(self, passes: int):
        """lib/mpc.py MAX_ITER inside mpcx_closed_loop_run: (window, rollout, QP) passes per step (stock configuration: 1)"""
        self._chk(self.lib.mpcx_set_linearisation_passes(self._ctx, int(passes)))
        self.lin_passes = int(passes)

    def set_step_fusion(self, on: bool):
        """mpcx_closed_loop_run without a graph: True (the default) = one launch per step for the plant update of the step before, the
        prediction and the warm-start rollout, where the run has none of the optional stages; False = a launch each, the rollout on the
        side stream.  The results are the same bits either way."""
        self._chk(self.lib.mpcx_set_step_fusion(self._ctx, 1 if on else 0))

    def set_qp_plain_rounds(self, on: bool):
        """stage-structured QP solver: True (the default) = rounds without a trial or polishing problem run the plain copies of the row
        passes; False = the generic text in every round.  The results are the same bits either way."""
        self._chk(self.lib.mpcx_qp_set_plain_rounds(self._ctx, 1 if on else 0))

    def profile_qp(self, enable: bool):
        """bracket every qp_kernel launch with HIP events on the context's stream (mpcx_profile_qp)"""
        self._chk(self.lib.mpcx_profile_qp(self._ctx, 1 if enable else 0))

    @_ordered
    def profile_qp_read(self):
        """(summed milliseconds, launches) of the bracketed qp_kernel launches since the last read"""
        ms, n = C.c_double(0.0), C.c_int32(0)
        self._chk(self.lib.mpcx_profile_qp_read(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ------------------------------------------------------------------ multi-GPU exchange (RCCL over xGMI)
    def comm_unique_id(self) -> bytes:
        """mpcx_comm_unique_id: rank 0 creates the id, the caller distributes it (sharding.init_comm broadcasts it)"""
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        rc = self.lib.mpcx_comm_unique_id(buf)
        if rc != 0:
            raise MpcxError('mpcx_comm_unique_id failed (%d)' % rc)
        return buf.raw

    def comm_init(self, world: int, rank: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), _lib.COMM_ID_BYTES)
        self._chk(self.lib.mpcx_comm_init(self._ctx, int(world), int(rank), buf))
        self.comm_world, self.comm_rank = int(world), int(rank)

    def comm_destroy(self):
        self._chk(self.lib.mpcx_comm_destroy(self._ctx))
        self.comm_world, self.comm_rank = 1, 0

    @_ordered
    def allgather_states(self, layout: int, local: torch.Tensor, out: torch.Tensor):
        """mpcx_allgather_states: local (n_inst, agents_local, 6) -> out, laid out as include/mpcx.h describes for `layout`"""
        n_inst, a_loc = int(local.shape[0]), int(local.shape[1])
        self._want(local, torch.float64, (n_inst, a_loc, 6), 'local'); self._want(out, torch.float64, None, 'out')
        world = getattr(self, 'comm_world', 1)
        if out.numel() != world * local.numel():
            raise MpcxError('allgather_states: out holds %d doubles, expected %d' % (out.numel(), world * local.numel()))
        self._chk(self.lib.mpcx_allgather_states(self._ctx, int(layout), n_inst, a_loc, _ptr(local), _ptr(out)))
        return out

    def synchronize(self):
        self.stream.synchronize()


class SearchModel:
    """Device copy of the tables `neighbor_function` needs (primitive id = position in the lists given)."""

    def __init__(self, ctx: Context, templates, last_pose, edge_cost, hp, hp_off):
        self.ctx = ctx
        tmpl_off = np.cumsum([0] + [len(t) for t in templates]).astype(np.int32)
        tmpl_xy = np.ascontiguousarray(np.concatenate([np.asarray(t)[:, :2] for t in templates]), np.float64)
        last_pose = np.ascontiguousarray(last_pose, np.float64)
        edge_cost = np.ascontiguousarray(edge_cost, np.float64)
        hp = np.ascontiguousarray(hp, np.float64).reshape(-1, 3)
        hp_off = np.ascontiguousarray(hp_off, np.int32)
        self.n_prim = len(templates)
        self.n_obst = len(hp_off) - 1
        self.n_pts_of = [len(t) for t in templates]      # collision-template points per primitive
        self.n_rows = int(len(hp))                        # half-plane rows of all obstacles
        self.edge_cost = edge_cost
        vp = C.c_void_p
        self._h = ctx.lib.mpcx_search_model_create(ctx._ctx, self.n_prim, vp(tmpl_off.ctypes.data), vp(tmpl_xy.ctypes.data),
                                                   vp(last_pose.ctypes.data), vp(edge_cost.ctypes.data), self.n_obst,
                                                   vp(hp_off.ctypes.data), vp(hp.ctypes.data))
        if not self._h:
            raise MpcxError('mpcx_search_model_create: %s' % ctx.lib.mpcx_last_error(ctx._ctx).decode())

    def close(self):
        if getattr(self, '_h', None):
            self.ctx.lib.mpcx_search_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
