#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the REFERENCE implementation.

Runs only in the build container (needs /root/reference, which never travels to the
GPU box).  It imports the reference's numpy-only modules exactly as its own scripts do
(cwd = main/scenarios, both /root/reference and /root/reference/main on sys.path) and
records inputs/outputs of the hot-path functions listed in SURVEY.md section 8(c)
(G1..G8).  `cvxpy` is not installable here, so an EMPTY module object is registered
under that name purely so that `import lib.mpc` succeeds; nothing of cvxpy is emulated
and `_linear_mpc_control` (the ECOS solve, mpc.py:138-208) is never called by this
stage.  Stage 2 (`--stage closedloop`) drives the reference's closed loop with
`lib.mpc._linear_mpc_control` replaced by this repo's CPU oracle QP (oracle/), to
harvest realistic pre-QP tensors (G9: these pin QP *inputs*; QP outputs are certified
by KKT residuals, see DESIGN.md "parity").

Only DATA is written (npz/json): no reference source, bytecode or pickle is copied.

usage:  python tests/golden/make_golden.py [--stage numpy|closedloop|...|horizons|moving_wide|all]
"""
import argparse
import json
import os
import sys
import types

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _enter_reference():
    os.environ.setdefault('MPLBACKEND', 'Agg')
    sys.dont_write_bytecode = True
    sys.path[:0] = [REF, os.path.join(REF, 'main')]
    os.chdir(os.path.join(REF, 'main', 'scenarios'))
    if 'cvxpy' not in sys.modules:
        sys.modules['cvxpy'] = types.ModuleType('cvxpy')  # empty: import-only placeholder


def _savez(name, **arrays):
    import numpy as np
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


def _savez_stable(name, **arrays):
    """as _savez, but byte-reproducible: np.savez_compressed stamps every member with the wall-clock time, this writes a fixed
    timestamp (np.load reads both alike)"""
    import io
    import zipfile
    import numpy as np
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


MP_SORTED = None  # primitive ids are defined by sorted name


def stage_numpy():
    import numpy as np
    from lib.motion_primitive import load_motion_primitives
    from lib.car_dimensions import BicycleModelDimensions, PriusDimensions
    from lib.linalg import create_2d_transform_mtx, transform_2d_pts
    from lib.maths import normalize_angle
    from lib.obstacles import check_collision, BoxObstacle, CircleObstacle
    from lib.trajectories import (resample_curve, calc_nearest_index_in_direction,
                                  car_trajectory_to_collision_point_trajectories)
    from lib.simulation import State, Simulation
    from lib.collision_avoidance import check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    from lib.moving_obstacles import MovingObstacleTIntersection
    from envs.intersection import intersection
    import lib.motion_primitive_search as mps_base
    import lib.motion_primitive_search_modified as mps_mod
    import lib.motion_primitive_search_multi_lane as mps_ml
    import lib.mpc as rmpc

    rng = np.random.default_rng(20241220)

    # ---------------- G1 primitives + car constants ----------------
    prim = {}
    meta = {}
    for version in ('bicycle_model', 'prius'):
        mps = load_motion_primitives(version)
        names = sorted(mps.keys())
        meta[version] = dict(names=names, glob_order=list(mps.keys()),
                             total_length=[float(mps[n].total_length) for n in names],
                             forward_speed=[float(mps[n].forward_speed) for n in names],
                             steering_angle=[float(mps[n].steering_angle) for n in names],
                             n_seconds=[float(mps[n].n_seconds) for n in names])
        for n in names:
            prim['%s/%s' % (version, n)] = np.asarray(mps[n].points, dtype=np.float64)
    cars = {}
    for cname, cd in (('bicycle_model', BicycleModelDimensions()), ('prius', PriusDimensions())):
        cars[cname] = dict(L=float(cd.distance_back_to_front_wheel), radius=float(cd.radius),
                           circle_centers=np.asarray(cd.circle_centers).tolist(),
                           bounding_box_size=list(map(float, cd.bounding_box_size)))
    meta['cars'] = cars
    with open(os.path.join(HERE, 'primitives_meta.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    _savez('primitives.npz', **prim)

    # ---------------- G2 collision templates, G3 scenarios ----------------
    bic = BicycleModelDimensions()
    pri = PriusDimensions()
    mps_b = load_motion_primitives('bicycle_model')
    mps_p = load_motion_primitives('prius')
    names_b = sorted(mps_b.keys())
    sc0 = intersection(start_pos=4, turn_indicator=1)
    tmpl = {}
    for tag, mps, cd in (('bicycle_model', mps_b, bic), ('prius', mps_p, pri)):
        s = mps_mod.MotionPrimitiveSearch(sc0, cd, mps, margin=cd.radius)
        for n, v in s._mp_collision_points.items():
            tmpl['%s/%s' % (tag, n)] = v
    _savez('templates.npz', **tmpl)

    scen = {}
    for sp in (1, 2, 3, 4):
        for ti in (1, 2, 3):
            sc = intersection(start_pos=sp, turn_indicator=ti)
            key = 'int_%d_%d' % (sp, ti)
            scen[key + '/start'] = np.array(sc.start, dtype=np.float64)
            scen[key + '/goal_point'] = np.array(sc.goal_point, dtype=np.float64)
            scen[key + '/goal_area'] = np.array([*sc.goal_area.xy1, *sc.goal_area.xy2], dtype=np.float64)
            scen[key + '/allowed_dtheta'] = np.array(sc.allowed_goal_theta_difference)
            kinds, params = [], []
            for o in sc.obstacles:
                if isinstance(o, BoxObstacle):
                    kinds.append(0)
                    params.append([*o.xy1, *o.xy2, float(o.hidden)])
                else:
                    kinds.append(1)
                    params.append([*o.xy_center, o.radius, 0.0, float(o.hidden)])
            scen[key + '/obst_kind'] = np.array(kinds, dtype=np.int32)
            scen[key + '/obst_param'] = np.array(params, dtype=np.float64)
            for tag, cd in (('bic', bic), ('pri', pri)):
                hps = [o.to_convex(margin=cd.radius) for o in sc.obstacles]
                scen[key + '/hp_%s' % tag] = np.concatenate(hps, axis=0).astype(np.float64)
                scen[key + '/hp_off'] = np.cumsum([0] + [len(h) for h in hps]).astype(np.int32)
    _savez('scenarios.npz', **scen)

    # ---------------- G5 full A* runs ----------------
    def run_case(mod, sc, cd, mps, **kw):
        names = sorted(mps.keys())
        s = mod.MotionPrimitiveSearch(sc, cd, mps, margin=cd.radius, **kw)
        cost, path, traj = s.run(debug=True)
        seq = [names.index(s._points_to_mp_names[a, b]) for a, b in zip(path[:-1], path[1:])]
        dbg = s.debug_data
        return s, dict(cost=np.array(cost), path=np.array(path, dtype=np.float64),
                       seq=np.array(seq, dtype=np.int32), traj=np.asarray(traj, dtype=np.float64),
                       dbg_node=np.array([d.node for d in dbg], dtype=np.float64),
                       dbg_pred=np.array([d.predecessor for d in dbg], dtype=np.float64),
                       dbg_g=np.array([d.g for d in dbg], dtype=np.float64),
                       dbg_h=np.array([d.h for d in dbg], dtype=np.float64))

    astar = {}
    log_nodes = []
    paths = {}
    for sp in (1, 2, 3, 4):
        for ti in (1, 2, 3):
            sc = intersection(start_pos=sp, turn_indicator=ti)
            s, out = run_case(mps_mod, sc, bic, mps_b)
            for k, v in out.items():
                astar['mod_bic_%d_%d/%s' % (sp, ti, k)] = v
            log_nodes.append(out['dbg_node'])
            paths[(sp, ti)] = out['traj']
    for sp, ti in ((4, 1), (1, 1), (3, 2), (2, 3)):
        sc = intersection(start_pos=sp, turn_indicator=ti)
        s, out = run_case(mps_base, sc, bic, mps_b)
        for k, v in out.items():
            astar['base_bic_%d_%d/%s' % (sp, ti, k)] = v
    for sp, ti in ((4, 1), (1, 2), (2, 3)):
        sc = intersection(start_pos=sp, turn_indicator=ti)
        s, out = run_case(mps_ml, sc, bic, mps_b)
        for k, v in out.items():
            astar['ml_bic_%d_%d/%s' % (sp, ti, k)] = v
    # non-default multi-lane weights exercise the obstacle / centre terms
    sc = intersection(start_pos=4, turn_indicator=1)
    s, out = run_case(mps_ml, sc, bic, mps_b, wh_obstacle=0.2, wh_center=0.1, wc_center=0.05)
    for k, v in out.items():
        astar['mlw_bic_4_1/%s' % k] = v
    for sp, ti in ((4, 1), (1, 2)):
        sc = intersection(start_pos=sp, turn_indicator=ti)
        try:
            s, out = run_case(mps_mod, sc, pri, mps_p)
            for k, v in out.items():
                astar['mod_pri_%d_%d/%s' % (sp, ti, k)] = v
        except Exception as e:  # degenerate prius primitives may not reach the goal
            print('prius case', sp, ti, 'raised', repr(e))
    _savez('astar_runs.npz', **astar)

    # ---------------- G4 neighbor_function on many nodes ----------------
    def expand_all(s, names, hps, node):
        """per-primitive collide flag + successor pose, with the reference's own helpers"""
        mtx = create_2d_transform_mtx(*node)
        flags = np.zeros(len(names), dtype=np.uint8)
        nbr = np.full((len(names), 3), np.nan)
        for i, n in enumerate(names):
            pts = transform_2d_pts(node[2], mtx, s._mp_collision_points[n])[:, :2].T
            flags[i] = any(check_collision(o, pts) for o in hps)
            x, y, th = np.squeeze(transform_2d_pts(node[2], mtx, np.atleast_2d(s._mps[n].points[-1]))).tolist()
            nbr[i] = (x, y, normalize_angle(th))
        return flags, nbr

    exp = {}
    for tag, cd, mps, sp, ti in (('bic', bic, mps_b, 4, 1), ('bic1', bic, mps_b, 1, 3), ('pri', pri, mps_p, 2, 1)):
        sc = intersection(start_pos=sp, turn_indicator=ti)
        names = sorted(mps.keys())
        s = mps_mod.MotionPrimitiveSearch(sc, cd, mps, margin=cd.radius)
        n_rand = 1500
        nodes = np.column_stack([rng.uniform(-38, 38, n_rand), rng.uniform(-38, 38, n_rand),
                                 rng.uniform(-np.pi, np.pi, n_rand)])
        # on-road nodes (lanes) so that many primitives are free
        lane = rng.choice([-3.0, 3.0], 600) + rng.normal(0, 0.6, 600)
        along = rng.uniform(-36, 36, 600)
        horiz = rng.random(600) < 0.5
        th = np.where(horiz, np.where(lane > 0, np.pi, 0.0), np.where(lane > 0, 0.5 * np.pi, -0.5 * np.pi))
        th = th + rng.normal(0, 0.25, 600)
        road = np.column_stack([np.where(horiz, along, lane), np.where(horiz, lane, along), th])
        extra = np.concatenate(log_nodes)[:: 3] if tag != 'pri' else np.zeros((0, 3))
        nodes = np.concatenate([nodes, road, extra, np.array([[0.0, 0.0, 0.3], [0.0, 0.0, -2.0]])])
        fl = np.zeros((len(nodes), len(names)), dtype=np.uint8)
        nb = np.zeros((len(nodes), len(names), 3))
        for k, nd in enumerate(nodes):
            fl[k], nb[k] = expand_all(s, names, s._obstacles_hp, tuple(nd.tolist()))
        exp[tag + '/nodes'] = nodes
        exp[tag + '/collide'] = fl
        exp[tag + '/nbr'] = nb
        exp[tag + '/scenario'] = np.array([sp, ti])
        # heuristics / goal tests of the three search variants on the same nodes
        sb = mps_base.MotionPrimitiveSearch(sc, cd, mps, margin=cd.radius)
        sm = mps_ml.MotionPrimitiveSearch(sc, cd, mps, margin=cd.radius)
        smw = mps_ml.MotionPrimitiveSearch(sc, cd, mps, margin=cd.radius, wh_obstacle=0.2, wh_center=0.1)
        exp[tag + '/h_base'] = np.array([sb.distance_to_goal(tuple(n.tolist())) for n in nodes])
        exp[tag + '/h_mod'] = np.array([s.distance_to_goal(tuple(n.tolist())) for n in nodes])
        exp[tag + '/h_ml'] = np.array([sm.distance_to_goal(tuple(n.tolist())) for n in nodes])
        exp[tag + '/h_mlw'] = np.array([smw.distance_to_goal(tuple(n.tolist())) for n in nodes])
        exp[tag + '/is_goal'] = np.array([s.is_goal(tuple(n.tolist())) for n in nodes], dtype=np.uint8)
    _savez('expand.npz', **exp)

    # ---------------- G7 MPC pre-QP helpers ----------------
    pre = {}
    vs = np.array([-5.0, -1.0, 0.0, 0.5, 3.0, 8.0, 30 / 3.6])
    phis = np.linspace(-3.5, 3.5, 15)
    lin_in, lin_A, lin_B, lin_C = [], [], [], []
    for v in vs:
        for ph in phis:
            for dl_ in (0.0, 0.2):
                A, B, C = rmpc._get_linear_model_matrix(v, ph, dl_, 0.2, 2.86)
                lin_in.append([v, ph, dl_, 0.2, 2.86]); lin_A.append(A); lin_B.append(B); lin_C.append(C)
    pre['lin/in'] = np.array(lin_in); pre['lin/A'] = np.array(lin_A)
    pre['lin/B'] = np.array(lin_B); pre['lin/C'] = np.array(lin_C)
    angs = np.linspace(-4, 4, 33)
    pre['xycost/angle'] = angs
    pre['xycost/M'] = np.array([rmpc._get_xy_cost_mtx_for_orientation(a) for a in angs])

    for T in (10, 13, 20):
        rmpc.T = T
        rmpc.Qf = np.diag([1.0, 1.0, 0.0, 0.5]) * T
        c_state, c_path, c_start, c_xref, c_tind, c_re, c_oa, c_od, c_xbar = [], [], [], [], [], [], [], [], []
        keys = sorted(paths.keys())
        for case in range(60):
            sp, ti = keys[case % len(keys)]
            full = paths[(sp, ti)].copy()
            rmpc.smooth_yaw(full[:, 2])
            n = len(full)
            cut = n if case % 3 else int(rng.integers(40, n))
            path = full[:cut]
            i0 = int(rng.integers(0, max(1, cut - 3)))
            if case % 7 == 0:
                i0 = max(0, cut - int(rng.integers(1, 30)))  # near the end: reaches_end rows
            lat = rng.normal(0, 0.3)
            yaw = path[i0, 2]
            st = State(x=path[i0, 0] - lat * np.sin(yaw), y=path[i0, 1] + lat * np.cos(yaw),
                       yaw=yaw + rng.normal(0, 0.05), v=float(rng.uniform(0, 30 / 3.6)) if case % 5 else 0.0)
            start = max(0, i0 - int(rng.integers(0, 4)))
            dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
            try:
                xref, tind, dref, re = rmpc._calc_ref_trajectory(st, path[:, 0], path[:, 1], path[:, 2], dl, 0.2, start, None)
            except Exception as e:
                print('ref case raised', repr(e)); continue
            oa = rng.uniform(-3, 2, T); od = rng.uniform(-0.9, 0.9, T) * (rng.random() < 0.8)
            xbar = rmpc._predict_motion([st.x, st.y, st.v, st.yaw], oa, od, xref, bic, 0.2)
            c_state.append([st.x, st.y, st.v, st.yaw]); c_path.append((sp, ti, cut)); c_start.append(start)
            c_xref.append(xref); c_tind.append(tind); c_re.append(re); c_oa.append(oa); c_od.append(od); c_xbar.append(xbar)
        pre['T%d/state' % T] = np.array(c_state); pre['T%d/path' % T] = np.array(c_path, dtype=np.int32)
        pre['T%d/start' % T] = np.array(c_start, dtype=np.int32); pre['T%d/xref' % T] = np.array(c_xref)
        pre['T%d/target_ind' % T] = np.array(c_tind, dtype=np.int32)
        pre['T%d/reaches_end' % T] = np.array(c_re, dtype=np.uint8)
        pre['T%d/oa' % T] = np.array(c_oa); pre['T%d/od' % T] = np.array(c_od); pre['T%d/xbar' % T] = np.array(c_xbar)
    rmpc.T = 13
    rmpc.Qf = np.diag([1.0, 1.0, 0.0, 0.5]) * 13
    # speed-reference variant: window of lib/mpc_with_speed.py (numpy-only part; xref[2,:] = cv[idx])
    import lib.mpc_with_speed as rmpcs
    for T in (13, 20):
        rmpcs.T = T
        ws_state, ws_cut, ws_start, ws_xref, ws_tind, ws_re, ws_cutoff = [], [], [], [], [], [], []
        full = paths[(4, 1)].copy()
        rmpc.smooth_yaw(full[:, 2])
        for case in range(24):
            cut = len(full) if case % 2 else int(rng.integers(100, len(full)))
            path = full[:cut]
            i0 = int(rng.integers(0, cut - 3))
            cutoff = 999 if case % 3 else int(rng.integers(i0, cut))
            cv = np.full(cut, rmpcs.MAX_SPEED)
            if cutoff != 999:
                cv[cutoff:] = 0
            st = State(x=path[i0, 0] + rng.normal(0, 0.2), y=path[i0, 1] + rng.normal(0, 0.2), yaw=path[i0, 2], v=float(rng.uniform(0, 8)))
            start = max(0, i0 - 2)
            dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
            xref, tind, dref, re = rmpcs._calc_ref_trajectory(st, path[:, 0], path[:, 1], cv, path[:, 2], dl, 0.2, start, None)
            ws_state.append([st.x, st.y, st.v, st.yaw]); ws_cut.append(cut); ws_start.append(start); ws_xref.append(xref)
            ws_tind.append(tind); ws_re.append(re); ws_cutoff.append(cutoff)
        pre['ws%d/state' % T] = np.array(ws_state); pre['ws%d/cut' % T] = np.array(ws_cut, dtype=np.int32)
        pre['ws%d/start' % T] = np.array(ws_start, dtype=np.int32); pre['ws%d/xref' % T] = np.array(ws_xref)
        pre['ws%d/target_ind' % T] = np.array(ws_tind, dtype=np.int32); pre['ws%d/reaches_end' % T] = np.array(ws_re, dtype=np.uint8)
        pre['ws%d/cutoff' % T] = np.array(ws_cutoff, dtype=np.int32)
    pre['ws/MAX_SPEED'] = np.array(rmpcs.MAX_SPEED)
    rmpcs.T = 13
    for (sp, ti), tr in paths.items():
        pre['path_%d_%d' % (sp, ti)] = tr  # raw A* trajectory (yaw NOT yet smoothed)
    # smooth_yaw vectors
    yy = np.concatenate([np.linspace(2.5, 3.6, 30) % (2 * np.pi) - np.pi, rng.uniform(-np.pi, np.pi, 40)])
    pre['smooth_yaw/in'] = yy.copy()
    pre['smooth_yaw/out'] = rmpc.smooth_yaw(yy.copy())
    _savez('mpc_pre.npz', **pre)

    # ---------------- G8 nearest index / resample / prediction / moving-car check ----------------
    mov = {}
    full = paths[(4, 1)]
    ni_in, ni_out = [], []
    for k in range(300):
        n = len(full)
        start = int(rng.integers(0, n))
        if k % 10 == 0:
            start = n - int(rng.integers(1, 4))
        i0 = min(n - 1, start + int(rng.integers(0, 25)))
        st = State(x=full[i0, 0] + rng.normal(0, 0.4), y=full[i0, 1] + rng.normal(0, 0.4), yaw=0.0, v=0.0)
        try:
            r = int(calc_nearest_index_in_direction(st, full[:, 0], full[:, 1], start_index=start, forward=True))
        except Exception:
            r = -1
        ni_in.append([st.x, st.y, start]); ni_out.append(r)
    mov['nearest/in'] = np.array(ni_in); mov['nearest/out'] = np.array(ni_out, dtype=np.int32)

    rs_cases = []
    for k, (v0, i0) in enumerate(((0.0, 0), (3.3, 100), (8.0, 250), (30 / 3.6, 10), (1.0, 600), (5.0, 655))):
        tr = full[i0:]
        if v0 < Simulation.MAX_SPEED:
            rdl = np.zeros((tr.shape[0],)) + rmpc.MAX_ACCEL
            rdl = np.cumsum(rdl) + v0
            rdl = 0.2 * np.minimum(rdl, Simulation.MAX_SPEED)
            out = resample_curve(tr, dl=rdl)
        else:
            out = resample_curve(tr, dl=0.2 * Simulation.MAX_SPEED)
        mov['resample/%d/in' % k] = np.array([v0, i0]); mov['resample/%d/out' % k] = out
    mov['resample/radius/out'] = resample_curve(mps_b['left3'].points.copy(), dl=bic.radius)

    pr_in, pr_out = [], []
    for k in range(40):
        six = [rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(0, 9), rng.uniform(-np.pi, np.pi),
               rng.uniform(-2, 2) * (k % 2), rng.uniform(-0.4, 0.4) * (k % 3 > 0)]
        o = np.vstack(MovingObstaclesPrediction(*six, sample_time=0.2, car_dimensions=bic).state_prediction(7.0)).T
        pr_in.append(six); pr_out.append(o)
    mov['predict/in'] = np.array(pr_in); mov['predict/out'] = np.array(pr_out)

    # scripted traffic of the stock scenario: the obstacle 6-tuples per step (scenario input data)
    obs = [MovingObstacleTIntersection(bic, direction=1, offset=2., turning=False, speed=25 / 3.6, dt=0.2),
           MovingObstacleTIntersection(bic, direction=-1, offset=4., turning=True, speed=25 / 3.6, dt=0.2)]
    tape = []
    for k in range(120):
        tape.append([list(map(float, o.get())) for o in obs])
        for o in obs:
            o.step()
    mov['traffic/tape'] = np.array(tape)  # (120, 2, 6)

    # moving-car collision chain, as main/scenarios/mpc_intersection.py:103-136 sequences it
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    margin = 4 * int(np.ceil(bic.radius / dl))
    mc_in, mc_obs, mc_hit, mc_cut, mc_nres = [], [], [], [], []
    for k in range(160):
        idx = int(rng.integers(0, len(full) - 5))
        v0 = float(rng.uniform(0, 30 / 3.6)) if k % 4 else 30 / 3.6
        traj = full[idx:]
        if v0 < Simulation.MAX_SPEED:
            rdl = np.zeros((traj.shape[0],)) + rmpc.MAX_ACCEL
            rdl = 0.2 * np.minimum(np.cumsum(rdl) + v0, Simulation.MAX_SPEED)
            tres = resample_curve(traj, dl=rdl)
        else:
            tres = resample_curve(traj, dl=0.2 * Simulation.MAX_SPEED)
        if k < 100:
            six = np.array(tape[int(rng.integers(0, 100))])
        else:
            nobs = int(rng.integers(1, 8))
            six = np.zeros((nobs, 6))
            for j in range(nobs):
                p = full[int(rng.integers(0, len(full)))]
                ang = rng.uniform(-np.pi, np.pi)
                d = rng.uniform(0, 40)
                sp_ = rng.uniform(0, 9)
                six[j] = [p[0] - d * np.cos(ang), p[1] - d * np.sin(ang), sp_, ang, rng.uniform(-1, 1), rng.uniform(-0.3, 0.3)]
        trajs = [np.vstack(MovingObstaclesPrediction(*s6, sample_time=0.2, car_dimensions=bic).state_prediction(7.0)).T
                 for s6 in six]
        hit = check_collision_moving_cars(bic, tres, traj, trajs, frame_window=20)
        if hit is None:
            mc_hit.append([np.nan, np.nan, -1]); mc_cut.append(len(full))
        else:
            cut = get_cutoff_curve_by_position_idx(full, hit[0], hit[1]) - margin
            cut = max(idx + 1, cut)
            mc_hit.append([hit[0], hit[1], hit[2]]); mc_cut.append(int(cut))
        pad = np.full((7, 6), np.nan); pad[:len(six)] = six
        mc_in.append([idx, v0, len(six)]); mc_obs.append(pad); mc_nres.append(len(tres))
    mov['moving/in'] = np.array(mc_in); mov['moving/obs'] = np.array(mc_obs)
    mov['moving/hit'] = np.array(mc_hit); mov['moving/cut'] = np.array(mc_cut, dtype=np.int32)
    mov['moving/nres'] = np.array(mc_nres, dtype=np.int32)
    mov['moving/margin'] = np.array(margin)
    _savez('moving.npz', **mov)


def stage_closedloop(max_iter=1, horizons=(10, 13, 20), name='closedloop.npz', max_steps=400, save=_savez):
    """G9: reference closed loop (mpc_intersection.py:95-159 sequence) with the oracle QP in place of ECOS.
    max_iter > 1 (closedloop_iter2.npz): the reference's successive linearisation, mpc.py:226-237 -- MAX_ITER passes per step, the
    reference window of every pass after the first spaced by the previous pass's speeds (`ov`), its rollout made with the previous
    pass's inputs; one record per QP call (MAX_ITER per step)."""
    import numpy as np
    sys.path.insert(0, REPO)
    from oracle import oracle_py as orc
    from lib.motion_primitive import load_motion_primitives
    from lib.car_dimensions import BicycleModelDimensions
    from lib.trajectories import resample_curve, calc_nearest_index_in_direction
    from lib.simulation import State, Simulation, HistorySimulation
    from lib.collision_avoidance import check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    from lib.moving_obstacles import MovingObstacleTIntersection
    from envs.intersection import intersection
    from lib.motion_primitive_search_modified import MotionPrimitiveSearch
    import lib.mpc as rmpc

    out = {}
    rmpc.MAX_ITER = max_iter
    for T in horizons:
        rmpc.T = T
        rmpc.Qf = np.diag([1.0, 1.0, 0.0, 0.5]) * T
        params = orc.MpcParams(T=T)
        rec = dict(x0=[], xref=[], xbar=[], re=[], oa=[], od=[], ox=[], status=[], target=[], hit=[], cut=[],
                   state=[], ctrl=[], tidx=[])

        def oracle_qp(xref, xbar, x0, dref, reaches_end, dt, car_dimensions):
            sol = orc.qp_solve(params, np.asarray(x0, float), xref, xbar, np.asarray(reaches_end, np.uint8))
            rec['x0'].append(np.asarray(x0, float)); rec['xref'].append(xref.copy()); rec['xbar'].append(xbar.copy())
            rec['re'].append(np.asarray(reaches_end, np.uint8))
            rec['status'].append(sol.status)
            if sol.status != 0:
                rec['oa'].append(np.full(T, np.nan)); rec['od'].append(np.full(T, np.nan)); rec['ox'].append(np.full((4, T + 1), np.nan))
                return None, None, None, None, None, None
            rec['oa'].append(sol.u[0].copy()); rec['od'].append(sol.u[1].copy()); rec['ox'].append(sol.x.copy())
            return sol.u[0].copy(), sol.u[1].copy(), sol.x[0].copy(), sol.x[1].copy(), sol.x[3].copy(), sol.x[2].copy()

        rmpc._linear_mpc_control = oracle_qp
        DT = 0.2
        mps = load_motion_primitives(version='bicycle_model')
        cd = BicycleModelDimensions(skip_back_circle_collision_checking=False)
        scenario = intersection(start_pos=4, turn_indicator=1)
        moving = [MovingObstacleTIntersection(cd, direction=1, offset=2., turning=False, speed=25 / 3.6, dt=DT),
                  MovingObstacleTIntersection(cd, direction=-1, offset=4., turning=True, speed=25 / 3.6, dt=DT)]
        search = MotionPrimitiveSearch(scenario, cd, mps, margin=cd.radius)
        _, _, full = search.run(debug=False)
        dl = np.linalg.norm(full[0, :2] - full[1, :2])
        mpc = rmpc.MPC(cx=full[:, 0], cy=full[:, 1], cyaw=full[:, 2], dl=dl, dt=DT, car_dimensions=cd)
        state = State(x=full[0, 0], y=full[0, 1], yaw=full[0, 2], v=0.0)
        sim = HistorySimulation(car_dimensions=cd, sample_time=DT, initial_state=state)
        margin = 4 * int(np.ceil(cd.radius / dl))
        tidx = 0
        tmp = None
        for i in range(max_steps):
            if mpc.is_goal(state):
                break
            if tmp is None or np.any(tmp[tidx, :] != tmp[-1, :]):
                tidx = calc_nearest_index_in_direction(state, full[:, 0], full[:, 1], start_index=tidx, forward=True)
            tres = traj = full[tidx:]
            if state.v < Simulation.MAX_SPEED:
                rdl = np.zeros((tres.shape[0],)) + rmpc.MAX_ACCEL
                rdl = DT * np.minimum(np.cumsum(rdl) + state.v, Simulation.MAX_SPEED)
                tres = resample_curve(tres, dl=rdl)
            else:
                tres = resample_curve(tres, dl=DT * Simulation.MAX_SPEED)
            trajs = [np.vstack(MovingObstaclesPrediction(*o.get(), sample_time=DT, car_dimensions=cd).state_prediction(7.)).T
                     for o in moving]
            hit = check_collision_moving_cars(cd, tres, traj, trajs, frame_window=20)
            if hit is not None:
                cut = get_cutoff_curve_by_position_idx(full, hit[0], hit[1]) - margin
                cut = max(tidx + 1, cut)
                tmp = full[:cut]
                rec['hit'].append([hit[0], hit[1], hit[2]]); rec['cut'].append(int(cut))
            else:
                tmp = full
                rec['hit'].append([np.nan, np.nan, -1]); rec['cut'].append(len(full))
            rec['state'].append([state.x, state.y, state.v, state.yaw]); rec['tidx'].append(int(tidx))
            mpc.set_trajectory_fromarray(tmp)
            delta, acc = mpc.step(state)
            rec['target'].append(int(mpc.target_ind)); rec['ctrl'].append([delta, acc])
            for o in moving:
                o.step()
            state = sim.step(a=acc, delta=delta, xref_deviation=mpc.get_current_xref_deviation())
        print('T=%d closed loop: %d steps, goal=%s' % (T, i, mpc.is_goal(state)))
        for k, v in rec.items():
            out['T%d/%s' % (T, k)] = np.array(v)
        out['T%d/full' % T] = full  # yaw column already smoothed in place by MPC.__init__
        out['T%d/steps' % T] = np.array(i)
    rmpc.MAX_ITER = 1
    save(name, **out)


HORIZONS = (1, 2, 9, 11, 14, 16, 17, 21, 24, 25, 30, 31, 32)


def stage_horizons():
    """mpc_pre_horizons.npz: the T%d/* window / rollout cases of mpc_pre.npz (same recipe and case mix: cut paths, starts near the
    end, v = 0, zero-steer warm starts) at the horizons the stock configuration does not use, 1 .. MPCX_T_MAX, plus the speed-reference
    window at T = 24 / 32; closedloop_horizons.npz: the stock closed loop of stage_closedloop at T = 16 / 24 / 32.  Own RNG seed; the
    A* paths are those recorded in mpc_pre.npz (path_%d_%d), so no search is rerun."""
    import numpy as np
    from lib.car_dimensions import BicycleModelDimensions
    from lib.simulation import State
    import lib.mpc as rmpc
    import lib.mpc_with_speed as rmpcs

    rng = np.random.default_rng(20261016)
    bic = BicycleModelDimensions()
    g = np.load(os.path.join(HERE, 'mpc_pre.npz'))
    paths = {(int(k.split('_')[1]), int(k.split('_')[2])): g[k] for k in g.files if k.startswith('path_')}
    pre = {}
    keys = sorted(paths.keys())
    for T in HORIZONS:
        rmpc.T = T
        rmpc.Qf = np.diag([1.0, 1.0, 0.0, 0.5]) * T
        c_state, c_path, c_start, c_xref, c_tind, c_re, c_oa, c_od, c_xbar = [], [], [], [], [], [], [], [], []
        for case in range(48):
            sp, ti = keys[case % len(keys)]
            full = paths[(sp, ti)].copy()
            rmpc.smooth_yaw(full[:, 2])
            n = len(full)
            cut = n if case % 3 else int(rng.integers(40, n))
            path = full[:cut]
            i0 = int(rng.integers(0, max(1, cut - 3)))
            if case % 7 == 0:
                i0 = max(0, cut - int(rng.integers(1, 30)))  # near the end: reaches_end rows
            lat = rng.normal(0, 0.3)
            yaw = path[i0, 2]
            st = State(x=path[i0, 0] - lat * np.sin(yaw), y=path[i0, 1] + lat * np.cos(yaw),
                       yaw=yaw + rng.normal(0, 0.05), v=float(rng.uniform(0, 30 / 3.6)) if case % 5 else 0.0)
            start = max(0, i0 - int(rng.integers(0, 4)))
            dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
            xref, tind, dref, re = rmpc._calc_ref_trajectory(st, path[:, 0], path[:, 1], path[:, 2], dl, 0.2, start, None)
            oa = rng.uniform(-3, 2, T); od = rng.uniform(-0.9, 0.9, T) * (rng.random() < 0.8)
            xbar = rmpc._predict_motion([st.x, st.y, st.v, st.yaw], oa, od, xref, bic, 0.2)
            c_state.append([st.x, st.y, st.v, st.yaw]); c_path.append((sp, ti, cut)); c_start.append(start)
            c_xref.append(xref); c_tind.append(tind); c_re.append(re); c_oa.append(oa); c_od.append(od); c_xbar.append(xbar)
        pre['T%d/state' % T] = np.array(c_state); pre['T%d/path' % T] = np.array(c_path, dtype=np.int32)
        pre['T%d/start' % T] = np.array(c_start, dtype=np.int32); pre['T%d/xref' % T] = np.array(c_xref)
        pre['T%d/target_ind' % T] = np.array(c_tind, dtype=np.int32)
        pre['T%d/reaches_end' % T] = np.array(c_re, dtype=np.uint8)
        pre['T%d/oa' % T] = np.array(c_oa); pre['T%d/od' % T] = np.array(c_od); pre['T%d/xbar' % T] = np.array(c_xbar)
    rmpc.T = 13
    rmpc.Qf = np.diag([1.0, 1.0, 0.0, 0.5]) * 13
    for T in (24, 32):
        rmpcs.T = T
        ws_state, ws_cut, ws_start, ws_xref, ws_tind, ws_re, ws_cutoff = [], [], [], [], [], [], []
        full = paths[(4, 1)].copy()
        rmpc.smooth_yaw(full[:, 2])
        for case in range(24):
            cut = len(full) if case % 2 else int(rng.integers(100, len(full)))
            path = full[:cut]
            i0 = int(rng.integers(0, cut - 3))
            cutoff = 999 if case % 3 else int(rng.integers(i0, cut))
            cv = np.full(cut, rmpcs.MAX_SPEED)
            if cutoff != 999:
                cv[cutoff:] = 0
            st = State(x=path[i0, 0] + rng.normal(0, 0.2), y=path[i0, 1] + rng.normal(0, 0.2), yaw=path[i0, 2], v=float(rng.uniform(0, 8)))
            start = max(0, i0 - 2)
            dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
            xref, tind, dref, re = rmpcs._calc_ref_trajectory(st, path[:, 0], path[:, 1], cv, path[:, 2], dl, 0.2, start, None)
            ws_state.append([st.x, st.y, st.v, st.yaw]); ws_cut.append(cut); ws_start.append(start); ws_xref.append(xref)
            ws_tind.append(tind); ws_re.append(re); ws_cutoff.append(cutoff)
        pre['ws%d/state' % T] = np.array(ws_state); pre['ws%d/cut' % T] = np.array(ws_cut, dtype=np.int32)
        pre['ws%d/start' % T] = np.array(ws_start, dtype=np.int32); pre['ws%d/xref' % T] = np.array(ws_xref)
        pre['ws%d/target_ind' % T] = np.array(ws_tind, dtype=np.int32); pre['ws%d/reaches_end' % T] = np.array(ws_re, dtype=np.uint8)
        pre['ws%d/cutoff' % T] = np.array(ws_cutoff, dtype=np.int32)
    pre['ws/MAX_SPEED'] = np.array(rmpcs.MAX_SPEED)
    rmpcs.T = 13
    _savez_stable('mpc_pre_horizons.npz', **pre)
    stage_closedloop(horizons=(16, 24, 32), name='closedloop_horizons.npz', save=_savez_stable)


def stage_onedisc():
    """moving_onedisc.npz: the moving-car conflict chain of moving.npz (same inputs) for a car with ONE collision disc
    (car_dimensions.py:51-75, skip_back_circle_collision_checking=True)."""
    import numpy as np
    from lib.car_dimensions import BicycleModelDimensions
    from lib.trajectories import resample_curve
    from lib.simulation import Simulation
    from lib.collision_avoidance import check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    import lib.mpc as rmpc
    mv = np.load(os.path.join(HERE, 'moving.npz'))
    full = np.load(os.path.join(HERE, 'mpc_pre.npz'))['path_4_1']
    one = BicycleModelDimensions(skip_back_circle_collision_checking=True)
    assert one.circle_centers.shape == (1, 2)
    margin = int(mv['moving/margin'])
    hits, cuts = [], []
    for k in range(len(mv['moving/in'])):
        idx, v0, nobs = mv['moving/in'][k]
        idx, nobs = int(idx), int(nobs)
        traj = full[idx:]
        if v0 < Simulation.MAX_SPEED:
            rdl = np.zeros((traj.shape[0],)) + rmpc.MAX_ACCEL
            rdl = 0.2 * np.minimum(np.cumsum(rdl) + v0, Simulation.MAX_SPEED)
            tres = resample_curve(traj, dl=rdl)
        else:
            tres = resample_curve(traj, dl=0.2 * Simulation.MAX_SPEED)
        assert len(tres) == mv['moving/nres'][k]
        trajs = [np.vstack(MovingObstaclesPrediction(*s6, sample_time=0.2, car_dimensions=one).state_prediction(7.0)).T
                 for s6 in mv['moving/obs'][k][:nobs]]
        hit = check_collision_moving_cars(one, tres, traj, trajs, frame_window=20)
        if hit is None:
            hits.append([np.nan, np.nan, -1]); cuts.append(len(full))
        else:
            cut = max(idx + 1, get_cutoff_curve_by_position_idx(full, hit[0], hit[1]) - margin)
            hits.append([hit[0], hit[1], hit[2]]); cuts.append(int(cut))
    _savez('moving_onedisc.npz', hit=np.array(hits), cut=np.array(cuts, dtype=np.int32), circle_centers=one.circle_centers)


WIDE_STEPS = (1, 2, 7, 35, 36, 50, 63, 64)
WIDE_WINDOWS = (0, 3, 20, 40, 70)
WIDE_CHUNK = 512            # obstacle disc positions the conflict-search kernel holds per pass (8 per lane)


def stage_moving_wide():
    """moving_wide.npz: the moving-car conflict chain of moving/* (same path, same car, same sequence of calls) beyond the stock
    point 7 obstacles / 35 frames / window 20: 8..16 obstacles, 1..64 predicted frames, windows 0..70.  Two parts, told apart by
    `kind`: 0 = random cases on the grid WIDE_STEPS x WIDE_WINDOWS, 1..6 = constructed cases (a)..(f) with standing obstacles placed on
    poses of the ego's own prediction, which fix WHICH obstacle rank holds the first row.  Every answer is the reference's; the
    asserts below are conditions on those answers (coverage of the fixture), not expectations of them."""
    import numpy as np
    from lib.car_dimensions import BicycleModelDimensions
    from lib.trajectories import resample_curve, car_trajectory_to_collision_point_trajectories
    from lib.simulation import Simulation
    from lib.collision_avoidance import check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    import lib.mpc as rmpc

    rng = np.random.default_rng(20261019)
    bic = BicycleModelDimensions()
    full = np.load(os.path.join(HERE, 'mpc_pre.npz'))['path_4_1']
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    margin = 4 * int(np.ceil(bic.radius / dl))
    assert margin == int(np.load(os.path.join(HERE, 'moving.npz'))['moving/margin'])
    NMAX = 16

    def ego_prediction(idx, v0):                    # main/scenarios/mpc_intersection.py:110-116
        traj = full[idx:]
        if v0 < Simulation.MAX_SPEED:
            rdl = np.zeros((traj.shape[0],)) + rmpc.MAX_ACCEL
            rdl = 0.2 * np.minimum(np.cumsum(rdl) + v0, Simulation.MAX_SPEED)
            return traj, resample_curve(traj, dl=rdl)
        return traj, resample_curve(traj, dl=0.2 * Simulation.MAX_SPEED)

    def predictions(six, steps):
        # `steps` frames: the horizon is half a sample short of 0.2 * steps, because np.arange(0, 0.2 * 63, 0.2) has 64 entries
        # (0.2 * 63 = 12.600000000000001); the frames themselves do not depend on the horizon
        trajs = [np.vstack(MovingObstaclesPrediction(*s6, sample_time=0.2, car_dimensions=bic).state_prediction(0.2 * steps - 0.1)).T
                 for s6 in six]
        assert all(len(t) == steps for t in trajs), (steps, [len(t) for t in trajs])
        return trajs

    rec = dict(inp=[], obs=[], hit=[], cut=[], nres=[], winner=[], kind=[], rank=[])

    def record(kind, rank, idx, v0, six, steps, window):
        traj, tres = ego_prediction(idx, v0)
        trajs = predictions(six, steps)
        hit = check_collision_moving_cars(bic, tres, traj, trajs, frame_window=window)
        winner = -1
        if hit is None:
            rec['hit'].append([np.nan, np.nan, -1]); rec['cut'].append(len(full))
        else:
            cut = max(idx + 1, get_cutoff_curve_by_position_idx(full, hit[0], hit[1]) - margin)
            rec['hit'].append([hit[0], hit[1], hit[2]]); rec['cut'].append(int(cut))
            for j in range(len(six)):               # the winner's rank: the shortest prefix of the obstacle list with the full answer
                if check_collision_moving_cars(bic, tres, traj, trajs[:j + 1], frame_window=window) == hit:
                    winner = j
                    break
            assert winner >= 0
        pad = np.full((NMAX, 6), np.nan); pad[:len(six)] = six
        rec['inp'].append([idx, v0, len(six), steps, window]); rec['obs'].append(pad); rec['nres'].append(len(tres))
        rec['winner'].append(winner); rec['kind'].append(kind); rec['rank'].append(rank)
        return winner

    # ---------------- random part ----------------
    grid = 1.0 / 4096           # obstacle states on a binary grid: they are inputs, and the file deflates to a third

    def far_obstacle():
        p = full[int(rng.integers(0, len(full)))]
        ang = rng.uniform(-np.pi, np.pi)
        d = rng.uniform(30, 80)
        return [p[0] - d * np.cos(ang), p[1] - d * np.sin(ang), rng.uniform(0, 9), rng.uniform(-np.pi, np.pi), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3)]

    def near_obstacle(idx):
        p = full[int(rng.integers(idx, len(full)))]
        ang = rng.uniform(-np.pi, np.pi)
        d = rng.uniform(0, 40)
        return [p[0] - d * np.cos(ang), p[1] - d * np.sin(ang), rng.uniform(0, 9), ang, rng.uniform(-1, 1), rng.uniform(-0.3, 0.3)]

    for steps in WIDE_STEPS:
        for window in WIDE_WINDOWS:
            for k in range(20):
                idx = int(rng.integers(0, len(full) - 5))
                v0 = float(rng.uniform(0, 30 / 3.6)) if k % 4 else 30 / 3.6
                nobs = int(rng.integers(8, NMAX + 1))
                n_near = 0 if k % 5 == 4 else 3
                six = np.array([far_obstacle() for _ in range(nobs - n_near)] + [near_obstacle(idx) for _ in range(n_near)])
                six = np.round(six / grid) * grid
                record(0, -1, idx, v0, six, steps, window)

    # ---------------- constructed part ----------------
    def far_row(j):
        return [300.0 + 10.0 * j, 300.0, 0.0, 0.0, 0.0, 0.0]        # >= 200 m from every path point

    def on_pose(pose, ahead=0.0):
        return [pose[0] + ahead * np.cos(pose[2]), pose[1] + ahead * np.sin(pose[2]), 0.0, pose[2], 0.0, 0.0]

    def constructed(kind, rank, idx, v0, near, steps):
        six = np.array([far_row(j) for j in range(NMAX)])
        for r, row in near.items():
            six[r] = row
        return record(kind, rank, idx, v0, six, steps, WIDE_WINDOWS[(rank if rank >= 0 else kind) % len(WIDE_WINDOWS)])

    def first_frame_and_disc(tres, row, steps):
        """(frame, agent disc) of the first row for ONE standing obstacle, written out plainly (for case (d) only: two obstacles that
        must share it)"""
        ag = [t[:, :2] for t in car_trajectory_to_collision_point_trajectories(tres, bic)]
        ob = [t[:, :2] for t in car_trajectory_to_collision_point_trajectories(predictions([row], steps)[0], bic)]
        for f in range(max(len(tres), steps)):
            for ca in range(2):
                for co in range(2):
                    if np.linalg.norm(ag[ca][min(f, len(tres) - 1)] - ob[co][min(f, steps - 1)]) <= 2 * bic.radius:
                        return f, ca
        return None

    IDX, V0 = 40, 30 / 3.6
    assert min(np.linalg.norm(full[:, :2] - np.array(far_row(j)[:2]), axis=1).min() for j in range(NMAX)) >= 200.0
    for steps in (35, 64):
        _, tres = ego_prediction(IDX, V0)
        assert len(tres) > 20
        for r in range(NMAX):                                               # (a)
            assert constructed(1, r, IDX, V0, {r: on_pose(tres[5])}, steps) == r
        assert constructed(2, -1, IDX, V0, {0: on_pose(tres[20]), 15: on_pose(tres[3])}, steps) == 15     # (b)
        assert constructed(3, -1, IDX, V0, {0: on_pose(tres[3]), 15: on_pose(tres[20])}, steps) == 0      # (c)
        for k in range(6, 20):                                              # (d): a pose where both obstacles meet the same frame and disc first
            lo, hi = on_pose(tres[k]), on_pose(tres[k], ahead=0.5)
            if first_frame_and_disc(tres, lo, steps) == first_frame_and_disc(tres, hi, steps) is not None:
                break
        else:
            raise AssertionError('(d): no pose on which both obstacles share their first frame and disc')
        n0 = len(rec['hit'])
        assert constructed(4, -1, IDX, V0, {2: lo, 13: hi}, steps) == 2
        constructed(4, -2, IDX, V0, {13: hi}, steps)                        # rank 13 alone: another answer, so the order is visible
        assert rec['hit'][n0] != rec['hit'][n0 + 1] and rec['winner'][n0 + 1] == 13
        idx_e = len(full) - 160                                            # (e): a prediction shorter than the obstacles', conflict on its last pose
        _, tres_e = ego_prediction(idx_e, V0)
        assert 5 < len(tres_e) < steps
        for r in range(NMAX):
            assert constructed(5, r, idx_e, V0, {r: on_pose(tres_e[-1])}, steps) == r
    _, tres_f = ego_prediction(0, V0)                                      # (f): a prediction longer than the obstacles'
    assert len(tres_f) > 30
    for r in range(NMAX):
        assert constructed(6, r, 0, V0, {r: on_pose(tres_f[30])}, 2) == r

    # ---------------- coverage conditions (on the reference's outputs) ----------------
    inp = np.array(rec['inp']); hit = np.array(rec['hit']); kind = np.array(rec['kind']); winner = np.array(rec['winner'], dtype=np.int32)
    nres = np.array(rec['nres'], dtype=np.int32)
    steps_, window_ = inp[:, 3].astype(int), inp[:, 4].astype(int)
    rnd = kind == 0
    for steps in WIDE_STEPS:
        for window in WIDE_WINDOWS:
            cell = rnd & (steps_ == steps) & (window_ == window)
            n_hit, n_free = int((hit[cell, 2] >= 0).sum()), int((hit[cell, 2] < 0).sum())
            assert n_hit >= 3 and n_free >= 2, (steps, window, n_hit, n_free)
    long_hits = rnd & (steps_ >= 35) & (hit[:, 2] >= 0)
    late = long_hits & (winner * steps_ * 2 >= WIDE_CHUNK)
    assert late.sum() >= 0.25 * long_hits.sum(), (int(late.sum()), int(long_hits.sum()))
    assert (nres[rnd] < steps_[rnd]).any() and (nres[rnd] == steps_[rnd]).any() and (nres[rnd] > steps_[rnd]).any()
    print('moving_wide: %d random cases (%d hits; steps >= 35: %d hits, %d with the winner in a later chunk), %d constructed'
          % (rnd.sum(), (hit[rnd, 2] >= 0).sum(), long_hits.sum(), late.sum(), (~rnd).sum()))
    _savez_stable('moving_wide.npz', **{'in': inp, 'obs': np.array(rec['obs']), 'hit': hit, 'cut': np.array(rec['cut'], dtype=np.int32),
                                        'nres': nres, 'winner_rank': winner, 'kind': np.array(kind, dtype=np.int32),
                                        'rank': np.array(rec['rank'], dtype=np.int32), 'margin': np.array(margin)})


def stage_traffic():
    """scripted actors of main/lib/moving_obstacles.py: get()/step() tapes for every class and branch"""
    import contextlib
    import io
    import numpy as np
    from lib.car_dimensions import BicycleModelDimensions
    from lib.moving_obstacles import (MovingObstacleArterial, MovingObstacleRoundabout, MovingObstacleTIntersection,
                                      calculate_steering_angle_for_radius)
    bic = BicycleModelDimensions()
    cases = {}
    k = 0
    for cls, name in ((MovingObstacleTIntersection, 'tint'), (MovingObstacleRoundabout, 'round')):
        for direction in (1, -1):
            for turning in (True, False):
                for offset, speed, dt in ((None, 25 / 3.6, 0.2), (1., 25 / 3.6, 0.2), (4., 20 / 3.6, 0.2), (0.5, 30 / 3.6, 0.1)):
                    cases['%s/%d' % (name, k)] = (cls, dict(direction=direction, turning=turning, offset=offset, speed=speed, dt=dt))
                    k += 1
    for x0, y0, offset, speed in ((3.0, -30.0, None, 10 / 3.6), (-2.5, -12.0, 2.0, 15 / 3.6)):
        cases['art/%d' % k] = (MovingObstacleArterial, dict(x_init=x0, y_init=y0, offset=offset, speed=speed, dt=0.2))
        k += 1
    out = {}
    meta = {}
    for key, (cls, kw) in cases.items():
        o = cls(bic, **kw)
        tape = []
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(150):
                tape.append(list(map(float, o.get())))
                o.step()
        out[key] = np.array(tape)
        meta[key] = dict(cls=cls.__name__, **{a: (None if v is None else (bool(v) if isinstance(v, bool) else float(v))) for a, v in kw.items()})
    out['arc_angle'] = np.array([calculate_steering_angle_for_radius(r) for r in (4.0, 5.0, 7.5)])
    _savez('traffic.npz', **out)
    with open(os.path.join(HERE, 'traffic_meta.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


def _world_arrays(sc):
    """Scenario -> plain arrays (obstacle classes are matched by name: some envs import them through another package path)"""
    import numpy as np
    ga = sc.goal_area
    kinds, params = [], []
    for o in sc.obstacles:
        if type(o).__name__ == 'BoxObstacle':
            kinds.append(0)
            params.append([*o.xy1, *o.xy2, float(o.hidden)])
        else:
            kinds.append(1)
            params.append([*o.xy_center, o.radius, 0.0, float(o.hidden)])
    return dict(start=np.array(sc.start, dtype=np.float64), goal_point=np.array(sc.goal_point, dtype=np.float64),
                goal_area=np.array([*ga.xy1, *ga.xy2], dtype=np.float64), allowed_dtheta=np.array(sc.allowed_goal_theta_difference),
                obst_kind=np.array(kinds, dtype=np.int32), obst_param=np.array(params, dtype=np.float64).reshape(-1, 5))


def stage_worlds():
    """every world the reference's main/envs/*.py can build, as obstacle-parameter tables (product data:
    mpc_for_av_at_intersection_amd/data/worlds.npz) + golden A* runs on the non-stock worlds / remaining search variants"""
    import contextlib
    import io
    import numpy as np
    from envs.intersection import intersection
    from envs.intersection_multi_lanes import intersection as intersection_ml
    from envs.roundabout import roundabout as roundabout_small
    from envs.roundabout_big import roundabout as roundabout_big
    from envs.t_intersection import t_intersection
    from lib.car_dimensions import BicycleModelDimensions
    from lib.motion_primitive import load_motion_primitives
    import lib.motion_primitive_search as mps_base
    import lib.motion_primitive_search_multi_lane as mps_ml
    import lib.motion_primitive_search_roundabout as mps_round
    import lib.motion_primitive_search_single_lane as mps_single
    worlds = {}
    made = {}

    def add(key, fn, **kw):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                sc = fn(**kw)
        except Exception as e:
            print('world', key, 'not buildable:', repr(e))
            return
        made[key] = sc
        for k, v in _world_arrays(sc).items():
            worlds['%s/%s' % (key, k)] = v

    for sp in (1, 2, 3, 4):
        for ti in (1, 2, 3, 4):
            if ti <= 3:
                add('intersection/%d_%d' % (sp, ti), intersection, start_pos=sp, turn_indicator=ti)
            add('t_intersection/%d_%d' % (sp, ti), t_intersection, start_pos=sp, turn_indicator=ti)
            add('roundabout/%d_%d' % (sp, ti), roundabout_small, start_pos=sp, turn_indicator=ti)
            add('roundabout_big/%d_%d' % (sp, ti), roundabout_big, start_pos=sp, turn_indicator=ti)
            if ti <= 3:
                for nl in (1, 2, 3):
                    for sl in range(1, nl + 1):
                        for gl in range(1, nl + 1):
                            add('intersection_multi_lanes/%d_%d_%d_%d_%d' % (sp, ti, sl, gl, nl), intersection_ml, start_pos=sp,
                                turn_indicator=ti, start_lane=sl, goal_lane=gl, number_of_lanes=nl)
    try:
        from envs.arterial_multi_lanes import ArterialMultiLanes
        for nl in (1, 2, 3, 4):
            for gl in range(1, nl + 1):
                add('arterial/%d_%d' % (nl, gl), lambda nl=nl, gl=gl: ArterialMultiLanes(num_lanes=nl, goal_lane=gl).create_scenario())
    except Exception as e:
        print('arterial not importable:', repr(e))
    path = os.path.join(REPO, 'mpc_for_av_at_intersection_amd', 'data', 'worlds.npz')
    np.savez_compressed(path, **worlds)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024), len(made), 'worlds')

    bic = BicycleModelDimensions()
    mps_b = load_motion_primitives('bicycle_model')

    def run_case(mod, sc, **kw):
        names = sorted(mps_b.keys())
        s = mod.MotionPrimitiveSearch(sc, bic, mps_b, margin=bic.radius, **kw)
        with contextlib.redirect_stdout(io.StringIO()):
            cost, path, traj = s.run(debug=True)
        seq = [names.index(s._points_to_mp_names[a, b]) for a, b in zip(path[:-1], path[1:])]
        dbg = s.debug_data
        return dict(cost=np.array(cost), path=np.array(path, dtype=np.float64), seq=np.array(seq, dtype=np.int32),
                    traj=np.asarray(traj, dtype=np.float64), dbg_node=np.array([d.node for d in dbg], dtype=np.float64),
                    dbg_g=np.array([d.g for d in dbg], dtype=np.float64), dbg_h=np.array([d.h for d in dbg], dtype=np.float64))

    runs = {}
    todo = [('round', mps_round, 'roundabout_big/1_1', {}), ('round', mps_round, 'roundabout_big/2_2', {}),
            ('round', mps_round, 'roundabout/1_3', {}), ('single', mps_single, 'intersection/4_1', {}),
            ('single', mps_single, 'intersection/2_3', {}), ('base', mps_base, 't_intersection/1_1', {}),
            ('base', mps_base, 't_intersection/2_2', {}), ('ml', mps_ml, 'intersection_multi_lanes/1_1_2_1_2', {}),
            ('ml', mps_ml, 'intersection_multi_lanes/3_2_1_2_3', dict(wh_obstacle=0.2, wc_center=0.02))]
    import signal

    def _too_long(signum, frame):
        raise TimeoutError('search exceeded its time box')
    signal.signal(signal.SIGALRM, _too_long)
    for tag, mod, key, kw in todo:
        if key not in made:
            print('skip', key)
            continue
        try:
            signal.alarm(240)
            try:
                out = run_case(mod, made[key], **kw)
            finally:
                signal.alarm(0)
        except BaseException as e:
            print('search', tag, key, 'raised', repr(e))
            continue
        print(tag, key, 'cost %.3f' % float(out['cost']), len(out['dbg_g']), 'expansions')
        for k, v in out.items():
            runs['%s|%s/%s' % (tag, key, k)] = v
    _savez('astar_worlds.npz', **runs)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--stage', default='numpy', choices=['numpy', 'closedloop', 'closedloop_iter2', 'onedisc', 'traffic', 'worlds', 'horizons', 'moving_wide', 'all'])
    a = ap.parse_args()
    _enter_reference()
    if a.stage in ('numpy', 'all'):
        stage_numpy()
    if a.stage in ('closedloop', 'all'):
        stage_closedloop()
    if a.stage in ('closedloop_iter2', 'all'):
        stage_closedloop(max_iter=2, horizons=(13,), name='closedloop_iter2.npz', max_steps=60)
    if a.stage in ('onedisc', 'all'):
        stage_onedisc()
    if a.stage in ('traffic', 'all'):
        stage_traffic()
    if a.stage in ('worlds', 'all'):
        stage_worlds()
    if a.stage in ('horizons', 'all'):          # reads the paths of mpc_pre.npz: after stage_numpy
        stage_horizons()
    if a.stage in ('moving_wide', 'all'):       # reads the path of mpc_pre.npz and the margin of moving.npz: after stage_numpy
        stage_moving_wide()
