"""Per-problem tuning rows (mpcx_set_instance_tuning, IntersectionBatch(tuning=...)) away from the stock parameters: the parameter sets
of tests/test_gpu_fullsize.py::test_sensitivity_sweep_as_one_batch, the 24 warm-started problems of helpers.horizon_problems with one
set each, their oracle and exact answers (computed once per horizon and shared), one-launch solves through Context.qp_solve, and the
coupled closed loop with one set per agent on the CPU oracle.  Used by tests/test_tuning_cpu.py and tests/test_gpu_tuning.py.

Row order: problem i carries set i % 16, so eight consecutive problems -- the eight lane groups of a stage-solver wavefront -- always sit
on eight different rows, in the order they lie, reversed, and tiled (problem j = problem j % 24 with row j % 16)."""
from types import SimpleNamespace

import numpy as np

from tests import helpers as H

N_SETS = 16
FIELDS = ('x', 'u', 'status', 'iters', 'kkt')


def parameter_sets(n=N_SETS, seed=5):
    """n keyword dicts from the sweep lattice of test_sensitivity_sweep_as_one_batch, drawn in that test's order"""
    rng = np.random.default_rng(seed)
    sets = []
    for _ in range(n):
        sets.append(dict(w_perp=float(rng.choice([1.0, 5.0, 20.0, 60.0])), w_para=float(rng.choice([0.2, 1.0, 4.0])),
                         R=(float(rng.choice([0.01, 0.1])), float(rng.choice([0.01, 0.5]))),
                         Rd=(float(rng.choice([0.01, 0.3])), float(rng.choice([0.2, 1.0, 3.0]))),
                         Q_v_yaw=(float(rng.choice([0.0, 1.0])), float(rng.choice([0.1, 0.5, 2.0]))),
                         Qf_base=(1.0, float(rng.choice([1.0, 2.0])), 0.0, float(rng.choice([0.5, 1.0]))),
                         max_accel=float(rng.choice([1.0, 2.0, 3.0])), max_decel=float(rng.choice([-10.0, -5.0])),
                         max_dsteer=float(np.deg2rad(rng.choice([15.0, 30.0, 60.0])))))
    return sets


def runtime_params(T, jerk=False, **kw):
    from mpc_for_av_at_intersection_amd.runtime import MpcParams
    return MpcParams.jerk(T=T, **kw) if jerk else MpcParams(T=T, **kw)


def oracle_params(T, jerk=False, **kw):
    from oracle import oracle_py as orc
    return orc.MpcParams.jerk(T=T, **kw) if jerk else orc.MpcParams(T=T, **kw)


_MIXED, _REF = {}, {}


def mixed(T, jerk=False):
    """the 24 problems of helpers.horizon_problems(T, n=12), problem i with set i % 16: .probs (list of (x0, xref, xbar, re, u_warm)),
    .arrays (the five stacked), .set_of, .base (stock runtime parameters of the model), .params / .oracle (per problem, runtime / oracle
    MpcParams), .rows ((24, 16) tuning rows).  Cached: nobody writes to it."""
    key = (T, bool(jerk))
    if key not in _MIXED:
        probs = H.horizon_problems(T, n=12)
        assert len(probs) == 24, len(probs)
        sets = parameter_sets()
        set_of = np.arange(len(probs)) % N_SETS
        params = [runtime_params(T, jerk, **sets[s]) for s in set_of]
        _MIXED[key] = SimpleNamespace(T=T, jerk=bool(jerk), probs=probs, arrays=H.stack_problems(probs), set_of=set_of, sets=sets,
                                      base=runtime_params(T, jerk), params=params, oracle=[oracle_params(T, jerk, **sets[s]) for s in set_of],
                                      rows=np.stack([p.tuning_row() for p in params]))
    return _MIXED[key]


def reference(T, jerk=False):
    """oracle and exact answers of mixed(T, jerk), each problem under its own set: .sol (QpSolution per problem), .status, .iters, .z (the
    oracle's point, packed as qp_literal packs it), .exact (qp_literal.exact_solution started from the oracle's active set: the minimiser is
    unique, so the start only decides the number of rounds), .dist (|oracle - exact| per problem).  Cached."""
    from oracle import oracle_py as orc
    from tests import qp_literal as QL
    key = (T, bool(jerk))
    if key not in _REF:
        m = mixed(T, jerk)
        sol = [orc.qp_solve(po, *q) for po, q in zip(m.oracle, m.probs)]
        z = [QL.pack(po, s.x, s.u) for po, s in zip(m.oracle, sol)]
        exact = [QL.exact_solution(po, q[0], q[1], q[2], q[3], zk) for po, q, zk in zip(m.oracle, m.probs, z)]
        _REF[key] = SimpleNamespace(sol=sol, status=np.array([s.status for s in sol]), iters=np.array([s.iters for s in sol]), z=z, exact=exact,
                                    dist=np.array([np.abs(zk - e['z']).max() for zk, e in zip(z, exact)]))
    return _REF[key]


def check_exact(ex):
    """the exact point is a KKT point of the literal problem to rounding (test_exact_active_set_solution_pins_the_oracle's side conditions)"""
    assert ex['eq'] < 1e-9 and ex['stat'] < 1e-7 * max(1.0, np.abs(ex['lam']).max() if len(ex['lam']) else 1.0), (ex['eq'], ex['stat'])
    assert (ex['lam'] >= -1e-7).all() and ex['slack'].min() > -1e-9


def pack_device(po, x, u):
    """a device solution as qp_literal packs it; the five-state model's fifth state -- which the kernels do not return -- rebuilt from the
    returned speeds and accelerations (tests/test_gpu_horizons.py::test_jerk_controller_at_long_horizons)"""
    from tests import qp_literal as QL
    if po.model == 1:
        x4 = (x[2, 1] - x[2, 0]) / po.dt - u[0, 0] + po.dt * np.concatenate([[0.0], np.cumsum(u[0])])
        x = np.vstack([x, x4])
    return QL.pack(po, x, u)


def take(arrays, idx):
    return [a[idx] for a in arrays]


def solve(ctx, solver, params, arrays, rows=None, hint=None):
    """one launch through Context.qp_solve: global parameters `params`, the forced `solver`, optional tuning rows (B, 16) and order hint
    (B,) (numpy).  Returns dict(x, u, status, iters, kkt) of numpy arrays.  Solver, hint and rows are back at 'auto' / None afterwards."""
    ctx.set_mpc_params(params)
    try:
        ctx.set_qp_solver(solver)
        ctx.set_instance_tuning(None if rows is None else ctx.f64(rows))
        ctx.set_qp_order_hint(None if hint is None else ctx.i32(hint))
        out = ctx.qp_solve(*(ctx.u8(a) if i == 3 else ctx.f64(a) for i, a in enumerate(arrays)))
        ctx.synchronize()
        return {k: out[k].cpu().numpy() for k in FIELDS}
    finally:
        ctx.set_qp_solver('auto')
        ctx.set_qp_order_hint(None)
        ctx.set_instance_tuning(None)


def assert_same_bits(a, b, what, ia=None, ib=None):
    """all five fields of launch a (rows ia) equal those of launch b (rows ib) bit for bit; the failure names the field and the problems"""
    for k in FIELDS:
        va, vb = (a[k] if ia is None else a[k][ia]), (b[k] if ib is None else b[k][ib])
        assert va.shape == vb.shape, (what, k)
        same = np.array([va[i].tobytes() == vb[i].tobytes() for i in range(len(va))])
        assert same.all(), '%s: %s differs for %d of %d problems, first %s' % (what, k, int((~same).sum()), len(same), np.flatnonzero(~same)[:8].tolist())


# ---------------------------------------------------------------- the coupled closed loop with one set per agent
LOOP = dict(B=2, A=8, T=20, steps=6, seed=0)
STOCK_PAIRS = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2))      # batch.stock_routes' order


def loop_scene(seed=LOOP['seed'], B=LOOP['B'], A=LOOP['A'], T=LOOP['T']):
    """batch.synthetic_batch's layout on the golden stock routes (no planning, no GPU): routes, dl, car, route_of_agent, start (B, A), and
    for agent q of the B * A the set q % 16 as keyword dict"""
    from mpc_for_av_at_intersection_amd.lib.car_dimensions import BicycleModelDimensions
    routes = [H.smoothed_path(*pr) for pr in STOCK_PAIRS]
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    rng = np.random.default_rng(seed)
    route_of = np.tile(np.arange(A) % len(routes), (B, 1))
    lens = np.array([len(r) for r in routes])[route_of]
    start = (rng.random((B, A)) * 0.35 * lens).astype(np.int64)
    sets = parameter_sets()
    return SimpleNamespace(routes=routes, dl=dl, cd=BicycleModelDimensions(), route_of=route_of, start=start, B=B, A=A, T=T,
                           sets=[sets[q % N_SETS] for q in range(B * A)])


def oracle_loop(sc, steps=LOOP['steps']):
    """the scene's closed loop on the CPU oracle, every agent under its own set, step for step as the device loop runs it (scene_helpers:
    every agent sees the start-of-step states of its instance mates with the controls applied in the step before).  Returns per step and
    agent (hit index or -1, iterations, status)."""
    from oracle import oracle_py as orc
    cd, A, P = sc.cd, sc.A, sc.B * sc.A
    L = cd.distance_back_to_front_wheel
    po = [oracle_params(sc.T, L=L, **s) for s in sc.sets]
    centers, radius = np.asarray(cd.circle_centers, dtype=np.float64).reshape(2, 2), float(cd.radius)
    margin = 4 * int(np.ceil(cd.radius / sc.dl))
    full = [sc.routes[r] for r in sc.route_of.reshape(-1)]
    start = sc.start.reshape(-1)
    state = np.array([[full[q][start[q], 0], full[q][start[q], 1], 0.0, full[q][start[q], 2]] for q in range(P)])
    applied = np.zeros((P, 2))          # (steer, accel)
    traj_idx, target, prev, u = [int(s) for s in start], [int(s) for s in start], [0] * P, [None] * P
    out = np.zeros((steps, P, 3), np.int64)
    for k in range(steps):
        pool = np.column_stack([state, applied[:, 1], applied[:, 0]])
        new_state, new_applied = state.copy(), applied.copy()
        for q in range(P):
            b = q // A
            rows = pool[[r for r in range(b * A, (b + 1) * A) if r != q]]
            r = orc.agent_step(po[q], full[q], sc.dl, state[q], rows, traj_idx[q], prev[q], target[q], u[q], centers, radius, margin)
            sol = r['sol']
            out[k, q] = (-1 if r['hit'] is None else int(r['hit'][2]), sol.iters, sol.status)
            if sol.status == 0:
                new_state[q] = orc.plant_step(po[q], state[q], sol.u[0, 0], sol.u[1, 0])
                new_applied[q] = (sol.u[1, 0], sol.u[0, 0])
                u[q] = sol.u.copy()
            traj_idx[q], target[q], prev[q] = int(r['traj_idx']), int(r['target_ind']), int(r['cut'])
        state, applied = new_state, new_applied
    return out
