#!/usr/bin/env python3
"""Generate tests/golden/closedloop_speedref.npz from the REFERENCE implementation: the closed loop of
main/scenarios/mpc_intersection_new_ref.py:90-159 -- the ego keeps its whole path and the speed reference is zeroed from the conflict
on (lib/mpc_with_speed.py:276-282) -- on path (1, 1) with the script's own two scripted cars, T = 13, with
`lib.mpc_with_speed._linear_mpc_control` (the ECOS solve) replaced by this repo's CPU oracle QP, exactly as make_golden.py's
closed-loop stage does for lib/mpc.py.

Runs only where the reference is checked out (see make_golden.py).  Only arrays are written: no reference text.

usage:  python tests/golden/make_golden_speedref.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REPO, _enter_reference, _savez_stable      # noqa: E402

NO_STOP = 999           # the script's "no conflict" value of cutoff_idx (mpc_intersection_new_ref.py:122,135)


def stage_speedref(name='closedloop_speedref.npz', max_steps=400):
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
    import lib.mpc_with_speed as rmpc

    T = 13
    assert rmpc.T == T and rmpc.MAX_ITER == 1
    params = orc.MpcParams(T=T, w_perp=10, w_para=1, Rd=(0.01, 1), Q_v_yaw=(20, 0.5), max_decel=-5)
    rec = dict(state=[], tidx=[], hit=[], stop=[], target=[], xref=[], re=[], ctrl=[], status=[], obs6=[], oa=[], od=[])

    def oracle_qp(xref, xbar, x0, dref, reaches_end, dt, car_dimensions):
        sol = orc.qp_solve(params, np.asarray(x0, float), xref, xbar, np.asarray(reaches_end, np.uint8))
        rec['xref'].append(xref.copy()); rec['re'].append(np.asarray(reaches_end, np.uint8)); rec['status'].append(sol.status)
        if sol.status != 0:
            rec['oa'].append(np.full(T, np.nan)); rec['od'].append(np.full(T, np.nan))
            return None, None, None, None, None, None
        rec['oa'].append(sol.u[0].copy()); rec['od'].append(sol.u[1].copy())
        return sol.u[0].copy(), sol.u[1].copy(), sol.x[0].copy(), sol.x[1].copy(), sol.x[3].copy(), sol.x[2].copy()

    rmpc._linear_mpc_control = oracle_qp
    DT = 0.2
    MAX_SPEED = 30 / 3.6
    mps = load_motion_primitives(version='bicycle_model')
    cd = BicycleModelDimensions(skip_back_circle_collision_checking=False)
    scenario = intersection(start_pos=1, turn_indicator=1)
    moving = [MovingObstacleTIntersection(cd, direction=1, offset=1., turning=False, speed=25 / 3.6, dt=DT),
              MovingObstacleTIntersection(cd, direction=-1, offset=4., turning=True, speed=25 / 3.6, dt=DT)]
    search = MotionPrimitiveSearch(scenario, cd, mps, margin=cd.radius)
    _, _, full = search.run(debug=False)
    dl = np.linalg.norm(full[0, :2] - full[1, :2])
    cv = np.full(full[:, 1].shape, MAX_SPEED)
    mpc = rmpc.MPC(cx=full[:, 0], cy=full[:, 1], cv=cv, cyaw=full[:, 2], dl=dl, dt=DT, car_dimensions=cd)
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
        rec['obs6'].append([list(o.get()) for o in moving])
        trajs = [np.vstack(MovingObstaclesPrediction(*o.get(), sample_time=DT, car_dimensions=cd).state_prediction(7.)).T
                 for o in moving]
        hit = check_collision_moving_cars(cd, tres, traj, trajs, frame_window=20)
        stop = NO_STOP
        if hit is not None:
            stop = get_cutoff_curve_by_position_idx(full, hit[0], hit[1]) - margin
            stop = max(tidx + 1, stop)
            rec['hit'].append([hit[0], hit[1], hit[2]])
        else:
            rec['hit'].append([np.nan, np.nan, -1])
        tmp = full
        rec['stop'].append(int(stop))
        rec['state'].append([state.x, state.y, state.v, state.yaw]); rec['tidx'].append(int(tidx))
        mpc.set_trajectory_fromarray(tmp, cutoff_idx=stop)
        delta, acc = mpc.step(state)
        rec['target'].append(int(mpc.target_ind)); rec['ctrl'].append([delta, acc])
        for o in moving:
            o.step()
        state = sim.step(a=acc, delta=delta, xref_deviation=mpc.get_current_xref_deviation())
    goal = bool(mpc.is_goal(state))
    n_stop = int(np.sum(np.array(rec['stop']) != NO_STOP))
    n_fail = int(np.sum(np.array(rec['status']) != 0))
    print('speed-reference closed loop on path (1, 1): %d path points, %d steps, goal=%s, %d steps with a stop index, %d failed solves, '
          'lowest speed after the start %.3f m/s' % (len(full), i, goal, n_stop, n_fail, min(s[2] for s in rec['state'][10:])))
    # what was measured when the fixture was introduced: whoever regenerates it notices drift
    assert len(full) == 720 and i == 88 and goal and n_stop == 40 and n_fail == 0, (len(full), i, goal, n_stop, n_fail)
    out = {k: np.array(v) for k, v in rec.items()}
    out['full'] = full          # yaw column already smoothed in place by MPC.__init__
    out['steps'] = np.array(i)
    out['v_ref'] = np.array(rmpc.MAX_SPEED)
    _savez_stable(name, **out)


if __name__ == '__main__':
    _enter_reference()
    stage_speedref()
