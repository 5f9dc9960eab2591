"""One closed-loop step of one ego in SPEED-REFERENCE mode, composed from the oracle's pieces: the body of the reference's newer scenario
script (main/scenarios/mpc_intersection_new_ref.py:90-159) with lib/mpc_with_speed.py's set_trajectory_fromarray(trajectory_full,
cutoff_idx) (:276-282).  The structure is oracle_py.agent_step's; what differs is what happens to the conflict: the path stays whole and
the speed profile cv = v_ref is zeroed from the stop index on -- unless the stop index is 999, the script's "no conflict" value, which
the reference's `if cutoff_idx != 999` also reads as "no stop" when it came from a real conflict."""
import numpy as np

from oracle import oracle_py as orc

NO_STOP = 999
V_REF = 25 / 3.6        # MAX_SPEED of lib/mpc_with_speed.py:36


def speed_params(T=13, **kw):
    """the constants of lib/mpc_with_speed.py:16-36 + the literals 10 / 1 of :161,165 as oracle parameters"""
    base = dict(T=T, w_perp=10, w_para=1, Rd=(0.01, 1), Q_v_yaw=(20, 0.5), max_decel=-5)
    base.update(kw)
    return orc.MpcParams(**base)


def speed_profile(n, stop, v_ref=V_REF, route_speed=None):
    """mpc_with_speed.py:280-282"""
    cv = np.full(n, float(v_ref)) if route_speed is None else np.array(route_speed, dtype=np.float64)
    if stop != NO_STOP:
        cv[stop:] = 0
    return cv


def agent_step(p, full, dl, state4, obs6, traj_idx, prev_len, target_ind, u_warm, centers, radius, cutoff_margin, v_ref=V_REF,
               pred_steps=35, frame_window=20, max_accel=2.0, route_speed=None):
    """prev_len: length of the previous tmp_trajectory: 0 / None before the first step, len(full) afterwards (tmp_trajectory =
    trajectory_full, :131,136).  Returns oracle_py.agent_step's dict with `stop` (999 = none) in place of `cut`."""
    full = np.ascontiguousarray(full, np.float64)
    x, y, v, yaw = state4
    advance = True
    if prev_len:                                                   # :98
        advance = bool(np.any(full[traj_idx] != full[prev_len - 1]))
    if advance:
        traj_idx = orc.nearest_index_in_direction(x, y, full[:, 0], full[:, 1], traj_idx)
        if traj_idx < 0:
            raise Exception("something wrong")
    traj = full[traj_idx:]
    if v < p.max_speed:                                            # :105-111
        rdl = np.cumsum(np.zeros(len(traj)) + max_accel) + v
        rdl = p.dt * np.minimum(rdl, p.max_speed)
        tres = orc.resample_curve(traj, rdl)
    else:
        tres = orc.resample_curve(traj, p.dt * p.max_speed)
    trajs = [orc.predict_obstacle(s6, p.dt, p.L, pred_steps) for s6 in obs6]
    hit = orc.check_collision_moving_cars(centers, radius, tres, traj, trajs, frame_window)
    stop = NO_STOP                                                 # :122-136
    if hit is not None:
        stop = orc.cutoff_idx(full, hit[0], hit[1]) - cutoff_margin
        stop = max(traj_idx + 1, stop)
    cv = speed_profile(len(full), stop, v_ref, route_speed)
    xref, target_ind, re = orc.calc_ref_trajectory(p, state4, full[:, 0], full[:, 1], full[:, 2], dl, target_ind, cv=cv)
    if target_ind < 0:
        raise Exception("something wrong")
    uw = np.zeros((2, p.T)) if u_warm is None else np.asarray(u_warm, float)
    xbar = orc.predict_motion(p, [x, y, v, yaw], uw[0], uw[1])
    sol = orc.qp_solve(p, [x, y, v, yaw], xref, xbar, re, uw)
    return dict(traj_idx=traj_idx, hit=hit, stop=stop, target_ind=target_ind, xref=xref, xbar=xbar, re=re, sol=sol, n_res=len(tres))
