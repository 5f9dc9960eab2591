/*
 * mpcx.h -- C ABI of libmpcx.so, the MI355X (gfx950) implementation of the per-timestep hot path of
 * SaeedRahmani/MPC_for_AV_at_Intersection.  The reference has no FFI of its own (pure Python); each entry
 * point below names the reference function(s) it replaces (paths relative to /root/reference/main) -- the
 * Python objects in mpc_for_av_at_intersection_amd/ present the reference's call surface on top of this ABI,
 * and INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns int32 status: 0 = OK, <0 = error
 *     (MPCX_E_*; text via mpcx_last_error()).  Solver non-convergence is per-instance DATA (status[] array),
 *     never an error code -- mirroring lib/mpc.py:196-206.
 *   - every array argument is a DEVICE pointer (HIP global memory, e.g. torch tensor.data_ptr()), float64 /
 *     int32 / uint8, C-contiguous, batch as the slowest index.  Caller owns every buffer.
 *   - launches go to the HIP stream given at mpcx_create (NULL = default stream); calls are asynchronous
 *     with respect to the host exactly like a kernel launch, the caller synchronises the stream.
 *   - one mpcx_ctx per host thread / stream; a ctx is not re-entrant.
 *   - what the reference's loop records ABOUT a run (History rows, the goal test that ends the loop) and the true clearance between the
 *     vehicles is the run log: mpcx_run_log, mpcx_closed_loop_run_logged, mpcx_record_step_batch.
 *   - the end of an agent's episode (the loop's `if mpc.is_goal(state): break`) is retirement at the goal: mpcx_retire,
 *     mpcx_closed_loop_run_retire; taking the arrived car out of everybody else's scene as well is departure: mpcx_scene,
 *     mpcx_closed_loop_run_scene; letting vehicles in on a schedule is admission: mpcx_admit, mpcx_closed_loop_run_admit; re-using a
 *     departed agent's slot for the next vehicle is respawn: mpcx_respawn, mpcx_closed_loop_run_respawn.  Who yields to whom at the crossing is
 *     right of way: mpcx_precedence, mpcx_closed_loop_run_precedence.  A route per vehicle of such a slot is mpcx_routes,
 *     mpcx_closed_loop_run_routes; mpcx_episode_summary reduces the episode table per instance and route.  Holding agents at the stop
 *     lines of a signalised crossing is mpcx_signals, mpcx_closed_loop_run_signals; lights that follow the demand are mpcx_actuation,
 *     mpcx_closed_loop_run_actuated; a speed advised ahead of a red light of a fixed plan is mpcx_advice, mpcx_closed_loop_run_advised.
 *     Connected agents, seen by the others on their last MPC solution instead of on their last controls, are mpcx_intent,
 *     mpcx_closed_loop_run_intent.  An unsignalised crossing whose manager admits only compatible movements is mpcx_reservation,
 *     mpcx_closed_loop_run_reserved.
 */
#ifndef MPCX_H
#define MPCX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCX_T_MAX 32            /* horizon capacity (2T lanes of one wavefront); every T in 1..32 is tested end to end */
#define MPCX_MAX_PRIM 16         /* motion primitives per search model */
#define MPCX_MAX_OBS 16          /* moving obstacles seen by one ego */
#define MPCX_PRED_STEPS_MAX 64   /* prediction horizon frames */
#define MPCX_MAX_REMAINING 1024  /* path points ahead of an agent mpcx_interaction_batch handles by default ... */
#define MPCX_MAX_PATH_LEN 4096   /* ... and at most, when mpcx_interaction_params.max_path_len asks for more */
#define MPCX_EGO_FRAMES_MAX 128  /* resampled ego poses: mpcx_moving_collision_batch; mpcx_interaction_batch handles capacity/4 - 32 */

enum {
    MPCX_OK = 0,
    MPCX_E_INVALID = -1,   /* bad argument (null pointer, size out of range, unsupported horizon) */
    MPCX_E_LAUNCH = -2,    /* HIP launch / runtime failure */
    MPCX_E_NODEVICE = -3   /* no usable GPU */
};

/* per-instance solver status (status[] outputs) */
enum { MPCX_QP_OPTIMAL = 0, MPCX_QP_MAXITER = 1, MPCX_QP_INFEASIBLE = 2, MPCX_QP_NUMERIC = 3 };

typedef struct mpcx_ctx mpcx_ctx;

/* lib/mpc.py:13-36 (config/mpc_config.json) + lib/simulation.py:23-25 + car_dimensions.py:82-107 */
typedef struct {
    int32_t T;          /* horizon, 1..MPCX_T_MAX */
    int32_t max_iter;   /* interior-point iteration cap */
    double dt, L;
    double w_perp, w_para;
    double R[2], Rd[2], Q_v_yaw[2];
    double Qf[4];       /* ALREADY multiplied by T (mpc.py:25) */
    double R_end[2];    /* diag(10,10) (mpc.py:178) */
    double max_speed, min_speed, max_accel, max_decel, max_steer, max_dsteer /* rad/s */;
    double tol;         /* KKT tolerance (relative) */
    int32_t model;      /* MPCX_MODEL_BICYCLE4 (lib/mpc.py) or MPCX_MODEL_JERK5 (lib/mpc_jerk.py:143-208: a fifth state integrates
                         * the acceleration input, its initial value is free; solved by the stage-structured solver whatever the batch) */
    int32_t reserved;
    double jerk_weight; /* jerk_penalty_weight, mpc_jerk.py:30 (MPCX_MODEL_JERK5 only) */
} mpcx_mpc_params;
enum { MPCX_MODEL_BICYCLE4 = 0, MPCX_MODEL_JERK5 = 1 };

mpcx_ctx *mpcx_create(int32_t device, void *hip_stream);
void mpcx_destroy(mpcx_ctx *ctx);
const char *mpcx_last_error(mpcx_ctx *ctx);
const char *mpcx_version(void);
int32_t mpcx_set_mpc_params(mpcx_ctx *ctx, const mpcx_mpc_params *p);

/* ---- lib/mpc.py:138-208 `_linear_mpc_control` (incl. :58-79 `_get_linear_model_matrix`, :129-135): the QP.
 * Solves B independent problems.  Outputs laid out as the reference's x.value / u.value:
 * x_out[b,0..3,:] = (x, y, v, yaw), u_out[b,0,:] = accel, u_out[b,1,:] = steer.  u_warm may be NULL (zeros).
 * status[b] != 0  <=>  the reference's "Cannot solve mpc" branch (outputs then hold the last iterate).
 * kkt[b,:] = (stationarity inf-norm, primal residual inf-norm, mean complementarity, unused). */
int32_t mpcx_qp_solve_batch(mpcx_ctx *ctx, int32_t B,
                            const double *x0 /*B,4: x,y,v,yaw*/, const double *xref /*B,4,T+1*/,
                            const double *xbar /*B,4,T+1*/, const uint8_t *reaches_end /*B,T+1*/,
                            const double *u_warm /*B,2,T or NULL*/,
                            double *x_out /*B,4,T+1*/, double *u_out /*B,2,T*/,
                            int32_t *status /*B*/, int32_t *iters /*B*/, double *kkt /*B,4*/);

/* ---- lib/mpc.py:86-109 `_calc_ref_trajectory` (+ trajectories.py:100-126) and :112-126 `_predict_motion`
 * (+ simulation.py:35-47, bicycle/main.py:28-41).  Paths are ragged: instance b tracks points
 * [path_off[b], path_off[b]+path_len[b]) of path_xyyaw (rows x,y,yaw; yaw already smooth_yaw'ed);
 * path_len[b] is the CURRENT (possibly cut) length, as after MPC.set_trajectory_fromarray.
 * target_ind is in-out (mpc.py:226).  target_ind[b] = -1 on the reference's Exception("something wrong").
 * path_v (NULL for lib/mpc.py) is the speed profile `cv` of lib/mpc_with_speed.py:85-108: xref[2,:] = cv[idx] (one value per path point,
 * shared by every agent on the path; a per-agent stop index goes through mpcx_mpc_prepare_batch_stop). */
int32_t mpcx_mpc_prepare_batch(mpcx_ctx *ctx, int32_t B, const double *state /*B,4: x,y,v,yaw*/,
                               const double *u_warm /*B,2,T or NULL*/,
                               const double *path_xyyaw /*npts,3*/, const double *path_v /*npts or NULL*/,
                               const int32_t *path_off /*B*/,
                               const int32_t *path_len /*B*/, double dl, int32_t *target_ind /*B in-out*/,
                               double *xref /*B,4,T+1*/, uint8_t *reaches_end /*B,T+1*/, double *xbar /*B,4,T+1*/);
/* the same for the second and later of MAX_ITER linearisation passes (lib/mpc.py:226-237 `_iterative_linear_mpc_control`): `ov`, the
 * speeds of the previous pass's solution (row 2 of its x, T+1 values per instance, instance b at ov + b * ov_stride), spaces the
 * reference window (mpc.py:95-98 with ov given) and u_warm = the previous pass's inputs makes the rollout (mpc.py:231).  ov = NULL is
 * mpcx_mpc_prepare_batch. */
int32_t mpcx_mpc_prepare_batch_ov(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm,
                                  const double *path_xyyaw, const double *path_v, const int32_t *path_off, const int32_t *path_len,
                                  double dl, int32_t *target_ind, const double *ov /*or NULL*/, int64_t ov_stride,
                                  double *xref, uint8_t *reaches_end, double *xbar);
/* the same with the STOP INDEX of lib/mpc_with_speed.py:276-282, `set_trajectory_fromarray(trajectory_full, cutoff_idx)` as
 * scenarios/mpc_intersection_new_ref.py:139 calls it: the path stays whole -- path_len[b] is the FULL length, the window is selected over
 * it and reaches_end is against its last point -- and the speed reference is cv = v_ref, 0 from stop_idx[b] on:
 *     xref[2, k] = idx_k >= stop_idx[b] ? 0 : (path_v ? path_v[idx_k] : v_ref).
 * The reference's quirk is kept: stop_idx[b] == MPCX_NO_STOP (999) means "no stop" (`if cutoff_idx != 999`, :281) even where it came
 * from a real conflict on a path of more than 999 points.  A stop index at or beyond the path length stops nothing either (that is what
 * mpcx_interaction_batch's cut_len is for an agent without a conflict: its output is a valid stop_idx as it stands).
 * len_seen (B or NULL, out) <- path_len[b]: the length of this step's tmp_trajectory, which the NEXT step's mpcx_interaction_batch takes as
 * prev_cut_len (mpc_intersection_new_ref.py:98,131,136: tmp_trajectory = trajectory_full, so its "do not advance" test only bites on the
 * last path point).  stop_idx = NULL: mpcx_mpc_prepare_batch_ov exactly (v_ref and len_seen are not read); else v_ref must be finite. */
#define MPCX_NO_STOP 999
int32_t mpcx_mpc_prepare_batch_stop(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm,
                                    const double *path_xyyaw, const double *path_v, const int32_t *path_off, const int32_t *path_len,
                                    double dl, int32_t *target_ind, const double *ov /*or NULL*/, int64_t ov_stride,
                                    const int32_t *stop_idx /*B or NULL*/, double v_ref, int32_t *len_seen /*B or NULL*/,
                                    double *xref, uint8_t *reaches_end, double *xbar);
/* lib/mpc.py:226 `for _ in range(MAX_ITER)` inside mpcx_closed_loop_run: passes >= 1 (default 1 = the stock mpc_config.json) */
int32_t mpcx_set_linearisation_passes(mpcx_ctx *ctx, int32_t passes);

/* ---- lib/motion_primitive_search.py:87-121 `neighbor_function` (+ obstacles.py:157-176 `check_collision`,
 * linalg.py:4-54, maths.py:4-10).  Model tables are copied to the device once by mpcx_search_model_create
 * (HOST pointers there).  primitive id = index in the arrays given (callers use sorted names).
 * A* nodes are compared by exact float equality and ordered by exact f-values (a_star.py:34-49): a search that must
 * replay the reference's pop order passes nodes_cs computed by the host's numpy (what linalg.py:4-22 calls), which
 * makes successor coordinates bit-identical to the reference; bulk expansion passes NULL. */
typedef struct mpcx_search_model mpcx_search_model;
mpcx_search_model *mpcx_search_model_create(mpcx_ctx *ctx, int32_t n_prim,
                                            const int32_t *tmpl_off /*n_prim+1*/, const double *tmpl_xy /*npts,2*/,
                                            const double *last_pose /*n_prim,3*/, const double *edge_cost /*n_prim*/,
                                            int32_t n_obst, const int32_t *hp_off /*n_obst+1*/, const double *hp /*rows,3*/);
void mpcx_search_model_destroy(mpcx_search_model *m);
int32_t mpcx_expand_batch(mpcx_ctx *ctx, const mpcx_search_model *m, int32_t n_nodes, const double *nodes /*n,3*/,
                          const double *nodes_cs /*n,2: cos,sin of nodes[:,2], or NULL = device sincos*/,
                          double *nbr /*n,P,3*/, double *cost /*n,P*/, uint8_t *collide /*n,P*/);

/* ---- lib/a_star.py:31-78 `AStar.run` + lib/motion_primitive_search.py:64-75,87-121 (is_goal, distance_to_goal, neighbor_function),
 * lib/motion_primitive_search_modified.py:80-89, lib/motion_primitive_search_multi_lane.py:56-108,155-181,226-237,
 * lib/motion_primitive_search_roundabout.py:131-157,212 and lib/motion_primitive_search_single_lane.py:145-162,218 for MANY independent
 * searches, open list and closed set resident on the device: one wavefront per search, no host work between expansions.  The pop order
 * is the reference's (tuples (g + h, g, node, predecessor) compared field by field, node identity = float equality), which needs the
 * reference's bits in every number: cos / sin of a node's heading come from a table the host fills with numpy (cs_theta ascending,
 * cs_val (cos, sin)): a heading missing from it ends the search with MPCX_ASTAR_MISS and the heading in buffers.miss.  Heuristic and
 * edge values are evaluated with un-fused IEEE operations; where the reference goes through libm pow (Python's x ** 2: one ulp from
 * x * x for ~0.08 % of arguments) or BLAS (np.linalg.norm) the device value can differ by an ulp, so the kernel LOGS every value it
 * used (successor log below), the host re-evaluates them with the reference's own expressions and hands the few that differ back in a
 * PER-SEARCH override table: rows (x, y, theta, kind) sorted as tuples inside each search's slice [ov_off, ov_off + ov_cnt) of
 * ov_key / ov_val; kind = -1: ov_val is h(node); kind = k >= 0: ov_val is the edge value of primitive k leaving `node`.  Overrides are
 * never consulted for MPCX_ASTAR_BASE (its arithmetic is exact on the device).  models / searches are HOST arrays; every pointer inside
 * mpcx_astar_buffers is a DEVICE pointer to caller-owned memory: heap n x heap_cap x 10 doubles, table n x table_cap x 8 doubles
 * FILLED WITH NaN (table_cap a power of two), log n x log_cap x 8 (node, g, h, predecessor per expansion: a_star.py:52), push_log
 * n x push_cap x 8 -- the successor log: (node, h, edge value, index of the expansion it came from, primitive id, g) per PUSH for
 * BASE / MODIFIED and per FREE successor for the other variants (h = NaN if the successor was not pushed) --, path n x path_cap x 3 and
 * path_prim n x path_cap (goal first, primitive that led to each node, -1 at the start), cost / miss / status / n_exp / n_push /
 * path_len n each.  A path longer than path_cap ends in MPCX_ASTAR_PATH_CAPACITY (nothing is truncated silently). */
enum { MPCX_ASTAR_BASE = 0, MPCX_ASTAR_MODIFIED = 1, MPCX_ASTAR_MULTI_LANE = 2, MPCX_ASTAR_ROUNDABOUT = 3, MPCX_ASTAR_SINGLE_LANE = 4 };
enum { MPCX_ASTAR_FOUND = 0, MPCX_ASTAR_EXHAUSTED = 1 /* "No solution found." */, MPCX_ASTAR_CAPACITY = 2, MPCX_ASTAR_MISS = 3,
       MPCX_ASTAR_PATH_CAPACITY = 4 };
typedef struct {
    double start[3];
    double goal_box[4];         /* BoxObstacle.xy1, xy2 of scenario.goal_area */
    double goal_point[3];
    double allowed_dtheta;      /* scenario.allowed_goal_theta_difference */
    double wh[5];               /* MULTI_LANE: wh_dist, wh_theta, wh_steering, wh_obstacle, wh_center (_multi_lane.py:24) */
    double wc[4];               /* MULTI_LANE: wc_dist, wc_steering, wc_obstacle, wc_center (_multi_lane.py:26) */
    const double *hp_norm;      /* DEVICE, one per half-plane row of the model: (a**2 + b**2)**0.5 as the host's Python evaluates it
                                 * (_multi_lane.py:95); needed by ROUNDABOUT / SINGLE_LANE and by MULTI_LANE with wh_obstacle != 0 */
    int32_t variant;            /* MPCX_ASTAR_BASE ... MPCX_ASTAR_SINGLE_LANE */
    int32_t max_expansions;
    int32_t ov_off, ov_cnt;     /* this search's slice of the override table */
} mpcx_astar_search;
typedef struct {
    int32_t heap_cap, table_cap, log_cap, push_cap, path_cap;
    double *heap, *table, *log, *push_log, *path, *cost, *miss;
    int32_t *status, *n_exp, *n_push, *path_len, *path_prim;
} mpcx_astar_buffers;
int32_t mpcx_astar_batch(mpcx_ctx *ctx, int32_t n_search, const mpcx_search_model *const *models, const mpcx_astar_search *searches,
                         int32_t n_cs, const double *cs_theta, const double *cs_val,
                         int32_t n_ov, const double *ov_key /*n_ov,4*/, const double *ov_val /*n_ov*/, const mpcx_astar_buffers *buffers);

/* ---- the same expansion for SEVERAL searches in one launch (many independent planners running concurrently): segment s = nodes
 * seg_off[s] .. seg_off[s+1]-1 of the node table (HOST array, n_seg+1 entries), expanded against models[s] (HOST array of
 * handles; all with the same number of primitives).  Outputs are laid out exactly as n_seg separate mpcx_expand_batch calls
 * on the segments would lay them out. */
int32_t mpcx_expand_multi_batch(mpcx_ctx *ctx, int32_t n_seg, const mpcx_search_model *const *models, const int32_t *seg_off,
                                const double *nodes /*n,3*/, const double *nodes_cs /*n,2 or NULL*/,
                                double *nbr /*n,P,3*/, double *cost /*n,P*/, uint8_t *collide /*n,P*/);

/* ---- lib/collision_avoidance.py:66-119 `check_collision_moving_cars` + `get_cutoff_curve_by_position_idx`,
 * lib/moving_obstacles_prediction.py:21-47, trajectories.py:58-86 `resample_curve`, and the caller sequence
 * scenarios/mpc_intersection.py:103-136.  P independent problems (one ego each).  Moving obstacles live in a
 * pool obs6[NOBS,6] of 6-tuples (x, y, v, yaw, a, steer) -- what MovingObstacle*.get() returns,
 * mpc_intersection.py:119-122; each is predicted once.  Problem p sees obstacles
 * obs_off[p] .. obs_off[p]+obs_cnt[p]-1 of the pool except index obs_skip[p] (-1 = none): an N-agent instance
 * puts its N agents in the pool and every agent skips itself.
 * path_cs holds cos/sin of the path yaw column (the host computes them once per path with the same libm the
 * reference uses, so disc centres match trajectories.py:11-37 bit for bit).
 * Outputs: traj_idx (in-out, the scenario's traj_agent_idx), hit_idx (-1 = None, else index on the remaining
 * path; -2 = limits exceeded: more path points ahead / resampled poses than the call's capacity (max_path_len) or more than
 * MPCX_MAX_OBS obstacles -- the agent's path is then left uncut, callers must treat it as an error (batch.check()); -3 = the reference's Exception("something wrong")), hit_xy, cut_len (length of the tmp_trajectory
 * handed to MPC.set_trajectory_fromarray). */
typedef struct {
    int32_t pred_steps;      /* len(arange(0, TIME_HORIZON, DT)) = 35 */
    int32_t frame_window;    /* 20 */
    int32_t cutoff_margin;   /* EXTRA_CUTOFF_MARGIN = 4*ceil(radius/dl) */
    int32_t max_path_len;    /* mpcx_interaction_batch: longest path of the call in points (sizes the kernel's LDS: state it exactly,
                              * resident wavefronts hide the kernel's latency); 0 = MPCX_MAX_REMAINING; at least 512, at most
                              * MPCX_MAX_PATH_LEN.  Resampled ego poses handled: capacity / 4 - 32 */
    double dt, L, radius;
    double circle_centers[4]; /* (x,y) of the 2 discs, car_dimensions.py:61-79 */
    double max_accel, max_speed;
    /* optional (NULL = off): per point of the path table, the arc length from the first point of ITS path (any running sum whose
     * differences inside one path are arc lengths will do), and a bound on how far such a difference can be from the reference's own
     * np.cumsum over the same steps (trajectories.py:72-79; a few n * 2^-53 * length: the host knows n and the length).  Paths are
     * constants of a run while every step of every agent re-derives step lengths and their running sum from the points: with the table
     * mpcx_interaction_batch takes floor(c_i / dl_i) from differences of its entries wherever c_i / dl_i is farther from an integer than
     * that bound (+ rounding) can move it, and falls back to the sequential sum over the points for an agent with a closer call --
     * identical outputs either way. */
    const double *path_cum;
    double path_cum_err;
    /* optional (NULL = off): per point k of the path table, the index (relative to the first point of ITS path) of the first point j <= k of
     * that path with sqrt(dx*dx + dy*dy) <= 0.001 from point k -- get_cutoff_curve_by_position_idx (collision_avoidance.py:107-119) asked
     * for the position of path point k, which is the only way mpc_intersection.py:125-131 ever asks it (collision_xy IS a path point).  A
     * property of the path alone (k itself unless the path has duplicate points), evaluated once on the host with the reference's own
     * expression; with it mpcx_interaction_batch looks the cut index up instead of scanning the path up to the conflict. */
    const int32_t *path_first_within;
    /* optional (plan_cnt = NULL: off; needs path_cum): the EGO PREDICTION of mpc_intersection.py:107-116 per path point.  Once the predicted
     * speed v + MAX_ACCEL (i + 1) has reached MAX_SPEED -- after four points from standstill with the stock constants -- resample_curve's dl
     * is the constant DT * MAX_SPEED, and as long as the few points before that stay in bucket 0 (checked per agent and step) the poses it
     * keeps from trajectory_full[t:] depend on t alone: row t of the tables holds their number (plan_cnt[t]; 0 = not tabulated), the disc
     * centres of the kept poses (plan_disc[t][plan_cap][4]: trajectories.py:11-37) and the boxes of the eight runs of frames the conflict
     * search culls with (plan_box[t][8][4] = xlo, xhi, ylo, yhi, inflated), all computed on the host with the reference's own numpy
     * expressions for plan_dl = DT * MAX_SPEED, plan_steps = pred_steps and the car's discs / radius.  path_disc[npts][4]: the disc centres
     * of every path point (the earliest-pose scan of collision_avoidance.py:88-104 reads them instead of rebuilding them).  An agent
     * whose step does not meet the condition takes the resampling pass as before: identical outputs either way. */
    const int32_t *plan_cnt;
    const double *plan_disc, *plan_box, *path_disc;
    int32_t plan_cap, plan_steps;
    double plan_dl, plan_radius;
} mpcx_interaction_params;
int32_t mpcx_interaction_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                               const double *state /*P,4*/,
                               const double *path_xyyaw /*npts,3*/, const double *path_cs /*npts,2: cos(yaw),sin(yaw)*/,
                               const int32_t *path_off /*P*/, const int32_t *path_len /*P (full length)*/,
                               const int32_t *prev_cut_len /*P or NULL*/,
                               int32_t n_obs_pool, const double *obs6 /*NOBS,6*/, const int32_t *obs_off /*P*/,
                               const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P or NULL*/,
                               int32_t *traj_idx /*P in-out*/, int32_t *hit_idx /*P*/, double *hit_xy /*P,2*/,
                               int32_t *cut_len /*P*/);

/* ---- lib/collision_avoidance.py:66-104 `check_collision_moving_cars` with the reference's own argument meaning:
 * problem p has an already-resampled ego trajectory ego_xyyaw[ego_off[p] .. +ego_len[p]) (traj_agent), a detailed
 * path (path_agent_detailed) and obs_cnt[p] already-predicted obstacle trajectories of exactly ip->pred_steps
 * poses each, stored as pool entries obs_off[p].. (traj_obstacles; only x, y, yaw are used by the reference).
 * *_cs = cos/sin of the yaw column, computed by the host.  hit_idx[p] = -1 for None, else the index on the
 * detailed path (the third element of the reference's return tuple), hit_xy = (x, y). -2 = limits exceeded. */
int32_t mpcx_moving_collision_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                                    const double *ego_xyyaw /*ne,3*/, const double *ego_cs /*ne,2*/,
                                    const int32_t *ego_off /*P*/, const int32_t *ego_len /*P*/,
                                    const double *path_xyyaw /*np,3*/, const double *path_cs /*np,2*/,
                                    const int32_t *path_off /*P*/, const int32_t *path_len /*P*/,
                                    int32_t n_obs_pool, const double *obs_xyyaw /*NOBS,steps,3*/, const double *obs_cs /*NOBS,steps,2*/,
                                    const int32_t *obs_off /*P*/, const int32_t *obs_cnt /*P*/,
                                    int32_t *hit_idx /*P*/, double *hit_xy /*P,2*/);

/* ---- lib/linalg.py:4-54 `create_2d_transform_mtx` + `transform_2d_pts` for n_items (pose, point-set) pairs:
 * item i maps points pts[pts_off[i] .. +pts_cnt[i]) (rows x, y, theta) to world space at nodes[i]; used for
 * motion_primitive_at / collision_checking_points_at / path_to_full_trajectory
 * (motion_primitive_search.py:77-85,123-135).  out rows beyond pts_cnt[i] are zero. */
int32_t mpcx_transform_batch(mpcx_ctx *ctx, int32_t n_items, int32_t max_pts, const double *nodes /*n,3*/,
                             const int32_t *pts_off /*n*/, const int32_t *pts_cnt /*n*/, const double *pts /*npts,3*/,
                             double *out /*n,max_pts,3*/);

/* ---- lib/collision_avoidance.py:107-119 `get_cutoff_curve_by_position_idx`: first index of each point list within
 * `radius` of xy[p]; -1 where the reference would return the input array ("no cutoff"). */
int32_t mpcx_cutoff_index_batch(mpcx_ctx *ctx, int32_t P, const double *pts /*npts,3*/, const int32_t *off /*P*/,
                                const int32_t *len /*P*/, const double *xy /*P,2*/, double radius, int32_t *out /*P*/);

/* ---- lib/moving_obstacles_prediction.py:21-47 `state_prediction`: poses (x, y, yaw) of `steps` Euler steps. */
int32_t mpcx_predict_obstacles_batch(mpcx_ctx *ctx, int32_t n, int32_t steps, double dt, double L,
                                     const double *obs6 /*n,6*/, double *out_xyyaw /*n,steps,3*/);

/* ---- self-test of the wave-level DPP helpers the kernels rely on (scans, shifts, reductions, reciprocal):
 * in64 = 64 doubles, out322 = results, layout documented at selftest_kernel in csrc/mpcx_misc.hip. */
int32_t mpcx_selftest_wave_ops(mpcx_ctx *ctx, const double *in64, double *out322);
/* f64 MFMA lane maps (v_mfma_f64_16x16x4) used by the Hessian build: D(16x16) = A(16x4, row-major) * B(4x16, row-major) */
int32_t mpcx_selftest_mfma(mpcx_ctx *ctx, const double *A64, const double *B64, double *D256);

/* ---- plant: lib/simulation.py:35-47 `Simulation.step` on B states with the first control of each solution;
 * failed instances (status != 0) get (previous steer, MAX_DECEL) as MPC.step does (mpc.py:294-297) and their row of
 * u is zeroed, which is the warm-start reset of mpc.py:222-224 for the next step. */
int32_t mpcx_plant_step_batch(mpcx_ctx *ctx, int32_t B, double *state /*B,4 in-out*/, double *u /*B,2,T in-out*/,
                              const int32_t *status /*B or NULL*/, double *applied /*B,2 in-out: (steer, accel)*/);

/* ---- scripted traffic: lib/moving_obstacles.py:16-231 (MovingObstacleTIntersection / MovingObstacleRoundabout /
 * MovingObstacleArterial) + bicycle/main.py:28-41, the cars of the reference's scenarios that never yield
 * (scenarios/mpc_intersection.py:42-45,118-122,155-156; mpc_roundabout.py:45-46; overtaking_cyclist_bidirectional_road.py:82).
 * One call = for every actor get() -- its 6-tuple (x, y, v, yaw, a = 0, steer) written to row pool_row[i] of obs6 -- followed by
 * step().  The step rule is csrc/mpcx_traffic_core.h: un-fused arithmetic in the reference's operation order, so the decision
 * columns (v, a, steer) are the host classes' bit for bit and the poses differ only by what the device's sincos / tan differ from
 * the host's libm.  MPCX_TRAFFIC_TAPE actors do no arithmetic: they copy row tape_off + cursor * tape_stride of the uploaded table
 * tape[rows][6] (cursor = 0, 1, ..., holding the last of its tape_rows rows) -- bit-exact replay of rows the host computed or recorded.
 * ALL mutable state is in actor_state (device, 4 doubles per actor: x, y, theta, counter -- the step counter, or the cursor of a
 * TAPE actor, as an integer-valued double): no call argument counts steps, a replayed hipGraph keeps advancing.
 * UNLIKE the other per-stage entry points this one is not asynchronous: the actor table and pool_row are device memory, so each call
 * first synchronises the stream and reads both back (80 bytes + 4 per actor) to check them -- kinds, TAPE actors inside the table, rows
 * inside the pool -- before it launches.  mpcx_closed_loop_run with traffic does the same (+ ego_row) ONCE PER CALL, before its first
 * launch: n_steps in one call pay it once, a caller that steps with n_steps = 1 pays it every step (and a graph replay likewise,
 * per call).  The kernels clamp every index all the same. */
enum { MPCX_TRAFFIC_TINTERSECTION = 0, MPCX_TRAFFIC_ROUNDABOUT = 1, MPCX_TRAFFIC_ARTERIAL = 2, MPCX_TRAFFIC_TAPE = 3 };
typedef struct {
    int32_t kind;        /* MPCX_TRAFFIC_* */
    int32_t direction;   /* +1: enters from the left (lane y = -3), -1: from the right (moving_obstacles.py:176-187) */
    int32_t turning;     /* `turning is True` of the constructor */
    int32_t tape_rows, tape_off, tape_stride;   /* TAPE: rows of this actor, its first row and the row distance between its steps */
    double speed;        /* m/s once the start delay is over */
    double offset;       /* start delay [s]: standing until counter > offset / counter_dt; <= 0 = none */
    double counter_dt;   /* what the delay is counted in: the constructor's dt, but always 0.2 for the roundabout class (:45) */
    double model_dt;     /* sample time of the plant */
    double L;            /* wheelbase of the plant */
    double x_turn;       /* TINTERSECTION: -10 / 12 */
    double arc;          /* ROUNDABOUT: arctan(2.86 / 5) as the host's libm gives it (moving_obstacles.py:16-25) */
} mpcx_traffic_actor;    /* 6 int32 + 7 doubles */
int32_t mpcx_traffic_step_batch(mpcx_ctx *ctx, int32_t n_actors, const mpcx_traffic_actor *actors, double *actor_state /*n,4 in-out*/,
                                const double *tape /*rows,6 or NULL without TAPE actors*/, int64_t tape_rows,
                                const int32_t *pool_row /*n*/, int32_t n_obs_pool, double *obs6 /*NOBS,6 out*/);

/* ---- the closed loop itself: scenarios/mpc_intersection.py:95-159 for P agents, n_steps times, with no host work
 * between steps.  One step = [pool row of agent q <- (x, y, v, yaw, accel, steer) of agent q, what MovingObstacle*.get()
 * returns; pool rows of the scripted actors <- their get(), mpcx_traffic_step_batch] -> mpcx_interaction_batch (prev_cut_len =
 * the cut_len of the previous step; zero = none yet) -> mpcx_mpc_prepare_batch (path_len = cut_len, warm start = u_sol) ->
 * mpcx_qp_solve_batch (warm start = u_sol, in place) -> mpcx_plant_step_batch.  Every agent is a moving obstacle for the agents
 * whose obs_off/obs_cnt window covers it.  Without traffic (n_actors = 0) the pool has exactly P rows and row q is agent q.  With
 * traffic the pool has pool_rows rows, agent q sits in row ego_row[q] and actor i in row actor_row[i] (the batch of this package
 * lays an instance out as [its A agents | its actors], so every window stays one contiguous run); the actors' step() takes
 * effect for the NEXT step, as o.step() at the end of the reference's loop body does (mpc_intersection.py:155-156).
 * All pointers are device pointers owned by the caller; the buffers
 * are the same ones the per-stage entry points take and hold the same values afterwards.
 * use_graph != 0 captures one step into a hipGraph on the context's stream (which must then not be the null
 * stream) and replays it n_steps times; the instantiated graph is cached in the context per descriptor. */
typedef struct {
    int32_t P;
    int32_t exchange;   /* 0: the pool obs6 is this rank's own P agents; MPCX_SHARD_AGENTS: agent-sharded multi-GPU layout, see below */
    double dl;
    double *state /*P,4*/, *applied /*P,2: (steer, accel)*/, *obs6 /*P,6 scratch (pool_rows,6 with traffic)*/;
    const double *path_xyyaw, *path_cs, *path_v /*or NULL*/;
    const int32_t *path_off /*P*/, *path_len /*P*/, *obs_off /*P*/, *obs_cnt /*P*/, *obs_skip /*P or NULL*/;
    int32_t *traj_idx /*P*/, *target_ind /*P*/, *hit_idx /*P*/, *cut_len /*P, zero-initialised*/;
    double *hit_xy /*P,2*/, *xref /*P,4,T+1*/, *xbar /*P,4,T+1*/;
    uint8_t *reaches_end /*P,T+1*/;
    double *x_sol /*P,4,T+1*/, *u_sol /*P,2,T zero-initialised*/;
    int32_t *status /*P*/, *iters /*P*/;
    double *kkt /*P,4*/;
    /* exchange == MPCX_SHARD_AGENTS only: this rank owns agents_local agents of each of n_inst instances (P = n_inst *
     * agents_local, agent order (instance, local agent)); the pool obs6 then has world * P rows laid out
     * [n_inst][world * agents_local][6] and is filled every step by mpcx_allgather_states from obs_local. */
    int32_t n_inst, agents_local;
    double *obs_local /*P,6 scratch*/;
    /* scripted traffic (n_actors = 0: none, the fields below are not read).  Refused together with exchange == MPCX_SHARD_AGENTS:
     * traffic is instance-local, the instance-sharded layout needs nothing. */
    int32_t n_actors, pool_rows /* rows of obs6: at least P + n_actors */;
    const mpcx_traffic_actor *actors /*n_actors*/;
    double *actor_state /*n_actors,4*/;
    const double *tape /*tape_rows,6 or NULL*/;
    const int32_t *actor_row /*n_actors*/, *ego_row /*P*/;
    int64_t tape_rows;
} mpcx_closed_loop;
int32_t mpcx_closed_loop_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                             int32_t n_steps, int32_t use_graph);
/* Step fusion (on by default).  A run of n steps without a graph on the local pool -- no scripted traffic, one linearisation pass, none of
 * the run log, retirement, scene, admission, respawn, routes, precedence, signals, actuation, advice, shared plans or reservations -- enqueues ONE launch per step for what
 * belongs to an agent alone: the plant update of the step before, the pack and prediction of its pool row and its warm-start rollout
 * (head_kernel); the run ends with the last step's plant update in a launch of its own.  Every buffer holds the same bits when the call
 * returns.  on = 0: the launch sequence without fusion (the rollout on the side stream beside the conflict search), for every run. */
int32_t mpcx_set_step_fusion(mpcx_ctx *ctx, int32_t on);
/* Plain rounds of the stage-structured QP solver (on by default).  In a round in which no problem of a wavefront is in its trial or a polish
 * round the solver runs second copies of its row passes, compiled without the selects that tell those rounds apart.  on = 0: the generic
 * text in every round.  The results are the same bits either way (tests/test_gpu_qp_plain_passes.py); the switch is there to show it. */
int32_t mpcx_qp_set_plain_rounds(mpcx_ctx *ctx, int32_t on);
/* run statistics accumulated on the device by every step of mpcx_closed_loop_run since the last reset (what the reference's scripts
 * print per run: solver failures; plus iteration counts): out4 = (agent-steps, interior-point iterations, failed solves, max iterations).
 * Synchronises the context's stream. */
int32_t mpcx_closed_loop_stats(mpcx_ctx *ctx, int64_t *out4 /*host*/, int32_t reset);
/* the QP work queue as the last step of mpcx_closed_loop_run with P agents left it (for tests of the queue's order): order[i] = the agent
 * in place i of the queue, keyslot[p] = (queue key << 24 | slot) under which the conflict search filed agent p (stale for an agent that was
 * not filed in that step).  Both host arrays of P words.  MPCX_E_INVALID if no closed loop has built a queue for at least P agents.
 * Synchronises the context's stream. */
int32_t mpcx_closed_loop_queue(mpcx_ctx *ctx, int32_t P, int32_t *order /*host, P*/, int32_t *keyslot /*host, P*/);
/* the obstacle prediction the last conflict search on this context worked from (for tests of the prediction): out[row][frame][disc][x, y],
 * rows x steps x 2 x 2 doubles, for the first `rows` pool rows and the pred_steps = `steps` of that call.  A row that was not predicted
 * (absent, or outside every window under scripted traffic) holds what an earlier call left.  MPCX_E_INVALID if no prediction that large
 * has been made.  Synchronises the context's stream. */
int32_t mpcx_interaction_prediction(mpcx_ctx *ctx, int32_t rows, int32_t steps, double *out /*host, rows*steps*4*/);

/* ---- the run log: what the reference's own loop produces ABOUT a run -- HistorySimulation's rows (lib/simulation.py:58-88 with
 * get_current_xref_deviation, lib/mpc.py:301-308), the end of the loop (mpc.is_goal, lib/mpc.py:310-326; mpc_intersection.py:97-98) --
 * plus the true distance between the vehicles, written per step and agent by ONE more kernel at the end of a step (record_kernel, after
 * the plant step), with no host work between steps, under plain enqueue and graph replay alike.  The rule is csrc/mpcx_record_core.h.
 * Row s of agent q (s = steps[q] when the step is recorded; dropped when s >= capacity, the outcome words advance all the same):
 *   rows_f64[s][q][0..7] = x, y, v, yaw (after the plant step), accel, steer (applied), xref_deviation (NaN after a failed solve),
 *                          clearance (min disc-to-disc distance - 2 radius to every other row of the agent's pool window at the START of
 *                          the step, the agent's own pose taken from its own pool row obs_skip[q]; +inf if there is nobody else)
 *   rows_i32[s][q][0..7] = traj_idx, target_ind, cut_len, hit_idx, status, iters, 0, 0
 * Per-agent outcome words (caller-initialised: steps 0, goal_step -1, contact_step -1, flags 0, min_clearance +inf):
 *   steps          rows offered so far (the write cursor: device memory, so a replayed graph keeps advancing)
 *   goal_step      steps taken when is_goal first held (= the reference's number of loop iterations), else -1; goal = last point of the
 *                  agent's full path, len(cx) = cut_len, target_ind and state as they stand after the step
 *   flags          bit 0: the agent has been clear of everybody (a step with clearance >= 0)
 *   min_clearance  minimum of clearance from the first clear step on;  contact_step: first step with clearance < 0 after it, else -1
 * 96 bytes per agent and step + 24 bytes per agent; capacity 0 = outcomes only (rows_* may then be NULL).  The library checks the
 * descriptor's pointers and alignment, it cannot check sizes: row buffers smaller than capacity x P x 8 elements, or outcome buffers
 * smaller than P, are the caller's fault (a write beyond them). */
typedef struct {
    int32_t capacity;    /* rows per agent */
    int32_t reserved;
    double goal_dis, stop_speed;   /* GOAL_DIS, STOP_SPEED of lib/mpc.py (1.5 m, 0.1389 m/s) */
    double *rows_f64 /*capacity,P,8*/;
    int32_t *rows_i32 /*capacity,P,8*/;
    int32_t *steps /*P*/, *goal_step /*P*/, *contact_step /*P*/, *flags /*P*/;
    double *min_clearance /*P*/;
} mpcx_run_log;
/* one step's record as a stage of its own (what mpcx_closed_loop_run_logged enqueues after the plant step): the buffers are the
 * closed loop's, after mpcx_plant_step_batch; obs6 the pool as the step's mpcx_interaction_batch saw it.  obs_skip is required. */
int32_t mpcx_record_step_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                               const double *state /*P,4*/, const double *applied /*P,2*/, const double *x_sol /*P,4,T+1*/,
                               const double *path_xyyaw /*npts,3*/, const int32_t *path_off /*P*/, const int32_t *path_len /*P (full length)*/,
                               const int32_t *target_ind /*P*/, const int32_t *cut_len /*P*/, const int32_t *traj_idx /*P*/,
                               const int32_t *hit_idx /*P*/, const int32_t *status /*P*/, const int32_t *iters /*P*/,
                               int32_t n_obs_pool, const double *obs6 /*NOBS,6*/, const int32_t *obs_off /*P*/,
                               const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P*/, const mpcx_run_log *log);
/* the same with the goal test's len(self.cx) given per agent (goal_len, P; NULL = cut_len, mpcx_record_step_batch itself): the
 * speed-reference loop keeps the whole path (goal_len = path_len) and logs its stop index in the cut_len column. */
int32_t mpcx_record_step_batch_goal(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                                    const double *state, const double *applied, const double *x_sol,
                                    const double *path_xyyaw, const int32_t *path_off, const int32_t *path_len,
                                    const int32_t *target_ind, const int32_t *cut_len, const int32_t *traj_idx,
                                    const int32_t *hit_idx, const int32_t *status, const int32_t *iters,
                                    int32_t n_obs_pool, const double *obs6, const int32_t *obs_off,
                                    const int32_t *obs_cnt, const int32_t *obs_skip, const int32_t *goal_len /*P or NULL*/,
                                    const mpcx_run_log *log);
/* mpcx_closed_loop_run with a run log: every step ends with the record stage.  The log travels beside the descriptor, not inside it:
 * mpcx_closed_loop keeps its size, so callers built against the struct as it was stay valid; the cached graph's key covers both.
 * log = NULL (or capacity 0 with every pointer NULL) is mpcx_closed_loop_run itself: the same launches with the same arguments.
 * Works with scripted traffic, with MPCX_SHARD_AGENTS (the pool is the all-gathered one) and with use_graph. */
int32_t mpcx_closed_loop_run_logged(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                    const mpcx_run_log *log, int32_t n_steps, int32_t use_graph);
/* ---- how the ego yields to a conflict.  The reference has two ways, and so has the loop:
 *   MPCX_STOP_CUT    scenarios/mpc_intersection.py: the path is cut in front of the conflict and the MPC runs into the path end.  What
 *                    mpcx_closed_loop_run / mpcx_closed_loop_run_logged do (they forward here with opts = NULL).
 *   MPCX_STOP_SPEED  scenarios/mpc_intersection_new_ref.py:90-159 with lib/mpc_with_speed.py: the path stays whole and the speed
 *                    reference is zeroed from the conflict on.  The conflict search runs as before; what it writes to cl->cut_len is now
 *                    the agent's STOP INDEX (the path length where there is no conflict: no stop; the work-queue key's "the cut moved" compares
 *                    it with the stop index of the previous step),
 *                    the window stage is mpcx_mpc_prepare_batch_stop with (cl->path_len, cl->cut_len as stop_idx, v_ref, prev_len as
 *                    len_seen), the record stage is mpcx_record_step_batch_goal with goal_len = cl->path_len and logs the stop index in
 *                    the cut_len column.  The conflict search's prev_cut_len is prev_len: caller-owned DEVICE memory, P int32,
 *                    ZERO-INITIALISED before the batch's first step ("no tmp_trajectory yet") and set to path_len by every step --
 *                    device memory, because a flag kept on the host would be frozen into a replayed graph.  cl->path_v, if given, is the
 *                    speed profile in front of the stop index instead of v_ref.  Pair it with the constants of lib/mpc_with_speed.py
 *                    (Q_v_yaw = (20, 0.5), w_perp 10, MAX_DECEL -5) in mpcx_set_mpc_params.
 * Scripted traffic, linearisation passes, per-instance tuning, use_graph, the run log and MPCX_SHARD_AGENTS work in both modes.  The
 * options travel beside the descriptor (mpcx_closed_loop keeps its size); the cached graph's key covers them.  An unknown stop_mode, a
 * v_ref that is not finite or prev_len = NULL in MPCX_STOP_SPEED is MPCX_E_INVALID before anything is launched. */
enum { MPCX_STOP_CUT = 0, MPCX_STOP_SPEED = 1 };
typedef struct {
    int32_t stop_mode;   /* MPCX_STOP_* */
    int32_t reserved;
    double v_ref;        /* MPCX_STOP_SPEED: the speed reference in front of the stop index (MAX_SPEED of lib/mpc_with_speed.py, 25 / 3.6) */
    int32_t *prev_len;   /* MPCX_STOP_SPEED: P, zero-initialised, see above */
} mpcx_closed_loop_opts;
int32_t mpcx_closed_loop_run_opts(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                  const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL = MPCX_STOP_CUT*/,
                                  int32_t n_steps, int32_t use_graph);

/* ---- retirement at the goal: the end of the reference's loop, `if mpc.is_goal(state): break` (scenarios/mpc_intersection.py:92-93,
 * mpc_intersection_new_ref.py:92-93), per agent and on the device.  done[q] != 0: agent q has arrived and is retired.  The last launch
 * of every step (retire_kernel, after the record stage; the rule is csrc/mpcx_retire_core.h) counts the step in steps_driven[q] and makes
 * the run log's goal test -- mpc.is_goal (lib/mpc.py:310-326) on the state after the plant step, len(cx) = this step's cut_len
 * (MPCX_STOP_SPEED: path_len), the same function the record stage calls -- for every agent still driving; on arrival it sets done[q] = 1
 * and zeroes applied[q].  From the next step on the agent
 *   - keeps its state row (the state the reference's loop ended with) and its applied row (0, 0): to the others it is a parked car;
 *   - is not filed in the QP work queue and not solved: u_sol, x_sol, status, iters, kkt, xref, xbar, reaches_end, target_ind, traj_idx,
 *     hit_idx, hit_xy and cut_len (MPCX_STOP_SPEED: prev_len too) stay bit for bit as its last driven step left them;
 *   - still has its pool row packed every step (from the frozen state and the zero controls): the other agents' view of the pool and of
 *     obs_off / obs_cnt / obs_skip does not change;
 *   - gets no further row in the run log (its cursor `steps` stops at goal_step; min_clearance and contact_step stay) and counts
 *     neither as an agent-step nor with iterations in mpcx_closed_loop_stats.
 * Scripted actors and agents still driving are unaffected.  With a run log attached and both started together, goal_step[q] ==
 * steps_driven[q] for every retired agent.  Both arrays are caller-owned DEVICE memory, zero-initialised (the goal test BEFORE the
 * first step, which only a path of fewer than 5 points can pass, is the caller's: set done[q] = 1 there); everything that changes is
 * device memory, so a replayed graph retires agents like a plain run.  The struct travels beside the descriptor (mpcx_closed_loop and
 * mpcx_closed_loop_opts keep their sizes); the cached graph's key covers it by value.
 * retire = NULL or an all-zero struct: no retirement, mpcx_closed_loop_run_opts itself -- the same launches with the same arguments.
 * MPCX_E_INVALID before anything is launched, whatever n_steps is: only one of the two pointers set; goal_dis or stop_speed not finite
 * or negative; P >= 2^24 (no queue order is built there); more than one linearisation pass (mpcx_set_linearisation_passes: the later
 * passes build their queue with the counting sort of mpcx_qp_solve_batch, which knows nothing of retired agents -- a follow-up).
 * Works with scripted traffic, the run log, both stop modes, use_graph and MPCX_SHARD_AGENTS (every rank retires its own agents). */
typedef struct {
    int32_t *done;         /* P, caller-owned, zero = driving; set to 1 by the step in which the agent arrives */
    int32_t *steps_driven; /* P, caller-owned: steps taken while driving = the reference's number of loop iterations once done */
    double goal_dis, stop_speed;   /* GOAL_DIS, STOP_SPEED of lib/mpc.py (with a run log: the log's) */
} mpcx_retire;
int32_t mpcx_closed_loop_run_retire(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                    const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                    const mpcx_retire *retire /*or NULL*/, int32_t n_steps, int32_t use_graph);

/* ---- departure: taking vehicles out of the scene.  absent[r] != 0: pool row r is not in the scene -- no other agent's conflict search
 * considers it (interaction_kernel builds the list of the PRESENT rows of its window, so a window with departed cars is a shorter
 * obstacle list, not the same list behind a test), the run log's clearance and contact of the other agents ignore it, and its prediction
 * is not computed (nothing reads it).  The defining property: for every driving agent a step with the mask equals a step whose obstacle
 * list is the agent's pool window minus its own row and the absent rows, relative order kept.
 * With a scene, retire_kernel sets absent[obs_skip[q]] -- agent q's own pool row, the same index with and without scripted traffic
 * (obs_skip[q] == ego_row[q] there) -- in the step in which q arrives.  It is the step's last launch, so the others see the car gone from
 * the NEXT step on.  The retired agent's own frozen buffers, done / steps_driven, the queue length and the statistics are exactly those of
 * retirement alone, and its pool row is still packed every step: it is simply not looked at.
 * The caller may preset words, e.g. a scripted actor's row, to hide that vehicle from everybody.  An agent whose own row is absent but
 * which still drives (done[q] == 0) is a GHOST: it sees the others, they do not see it, and its own clearance is still measured from
 * its own (packed) row.
 * absent is caller-owned DEVICE memory, n_rows int32 words, zero-initialised; everything that changes is device memory, so a replayed
 * graph departs agents like a plain run.  The struct travels beside the descriptor (no other struct changes size); the cached graph's key
 * covers it by value.  scene = NULL or an all-zero struct: mpcx_closed_loop_run_retire itself -- the same launches with the same arguments.
 * MPCX_E_INVALID ("scene: ...") before anything is launched, whatever n_steps is: n_rows is not the pool's row count (pool_rows with
 * scripted traffic, else P); a scene without retirement; a scene with MPCX_SHARD_AGENTS (a remote rank's mask would have to travel with
 * the all-gather -- a follow-up); obs_skip NULL, or an agent whose own row obs_skip[q] lies outside the pool (read back once per call, as
 * the row maps of scripted traffic are).  A window of more than 64 rows is beyond the kernel's capacity with a scene (hit_idx -2) however
 * many of its rows are absent.  Works with scripted traffic, the run log, both stop modes and use_graph. */
typedef struct {
    int32_t *absent;     /* n_rows, caller-owned, zero = in the scene */
    int32_t n_rows;      /* rows of the pool: pool_rows with scripted traffic, else P */
    int32_t reserved;
} mpcx_scene;
int32_t mpcx_closed_loop_run_scene(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                   const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                   const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                   int32_t n_steps, int32_t use_graph);

/* ---- admission: letting vehicles INTO the scene on a schedule, the counterpart of departure.  A scheduled agent waits in the state
 * retirement and departure already define -- done[q] = 1 and absent[obs_skip[q]] = 1, both preset by the caller: it is not solved, not
 * logged, not counted and not seen, and its buffers stay bit for bit as they were allocated, so that it starts like the first step of a
 * fresh batch.  wait[q] says when it asks to enter:
 *   -1   not scheduled, or already entered: the agent is not touched;
 *   > 0  steps still to wait: decremented once per step, nothing else;
 *   0    DUE: the agent asks to enter in this step.
 * A due agent is admitted iff its start pose (its state row: it never moved) has clearance >= gap -- the run log's clearance: two discs
 * per car, min distance - 2 radius -- to every BLOCKING row of its pool window obs_off .. + obs_cnt minus its own row.  A row blocks if it
 * is present at the start of the step (absent[r] == 0 as the previous step left it) or if it is the own row of another agent q' < q that
 * is also due in this step, whether or not q' itself gets in.  The second clause is the tie-break: the outcome does not depend on the order
 * in which lanes run and two cars due at one pose never enter together; the price is that q may wait one step longer than strictly
 * necessary.  The poses are those this step's pool will hold: an agent's state row, a scripted actor's get() row of this step (computed from
 * a copy of its state; the actor is not stepped).  A pool row that belongs to neither is nobody.
 * On admission done[q] = 0, absent[obs_skip[q]] = 0, wait[q] = -1 and entered_step[q] = *clock, the number of closed-loop steps completed
 * since admission was switched on -- a device word the stage advances once per step, so a replayed graph counts like a plain run.
 * The stage is two small launches (csrc/mpcx_admit.hip; the rule is csrc/mpcx_admit_core.h) and the FIRST thing a step does: the admitted
 * agent is driven, packed, predicted, seen and logged by this very step.  An agent whose own row lies outside the pool is never admitted
 * and never written.
 * All three arrays are caller-owned DEVICE memory.  The struct travels beside the descriptor (no other struct changes size); the cached
 * graph's key covers it by value.  admit = NULL or an all-zero struct: mpcx_closed_loop_run_scene itself -- the same launches with the same
 * arguments.  MPCX_E_INVALID ("admit: ...") before anything is launched, whatever n_steps is: admission without a scene (which in turn needs
 * retirement and refuses MPCX_SHARD_AGENTS); one of the three pointers NULL; gap not finite or negative.
 * Works with scripted traffic, the run log, both stop modes and use_graph. */
typedef struct {
    int32_t *wait;          /* P, caller-owned device memory: -1 not scheduled / entered, > 0 steps to wait, 0 due */
    int32_t *entered_step;  /* P, caller-owned: clock value at admission; caller-initialised (-1 for scheduled agents) */
    int32_t *clock;         /* 1 word, caller-owned, zero-initialised */
    int32_t reserved;
    double gap;             /* metres of clearance the entry needs; 0 = the car overlaps nobody */
} mpcx_admit;
int32_t mpcx_closed_loop_run_admit(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                   const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                   const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                   const mpcx_admit *admit /*or NULL*/, int32_t n_steps, int32_t use_graph);
/* one step's admission as a stage of its own (what mpcx_closed_loop_run_admit enqueues at the head of a step): done is mpcx_retire::done,
 * absent is mpcx_scene::absent over the n_obs_pool rows of the pool, obs_skip names the agents' own rows; the actors are those of
 * mpcx_traffic_step_batch (n_actors = 0: none) and are read, not stepped.  Needs no mpcx_set_mpc_params. */
int32_t mpcx_admit_step_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state /*P,4*/,
                              const int32_t *obs_off /*P*/, const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P*/,
                              int32_t *done /*P*/, int32_t n_obs_pool, int32_t *absent /*NOBS*/,
                              int32_t n_actors, const mpcx_traffic_actor *actors /*n_actors*/, const double *actor_state /*n_actors,4*/,
                              const double *tape /*rows,6 or NULL*/, int64_t tape_rows, const int32_t *actor_row /*n_actors*/,
                              const mpcx_admit *admit);

/* ---- respawn: re-using a departed agent's slot for the next vehicle, which makes retirement, departure and admission an OPEN intersection.
 * A slot (agent index q) serves a stream of `generations` vehicles, all on the slot's route from the slot's start pose.  The LAST launch of
 * every step (respawn_kernel, after retire_kernel; csrc/mpcx_respawn.hip, the rule is csrc/mpcx_respawn_core.h) looks at every agent that is
 * not driving.  Agent q HAS ARRIVED iff done[q] != 0, wait[q] == -1, entered_step[q] >= 0, served[q] < generations and its own row
 * obs_skip[q] lies inside the pool.  With `clock` = admission's word as this step's admission stage left it (already advanced: the index of
 * the NEXT step) the arrival, in this order,
 *   1. writes episode record g = served[q] of slot q:
 *        ep_i32[q][g][0..7] = entered_step, arrived_step = clock - 1, steps_driven, row_end = the run log's cursor steps[q] (-1 without a log),
 *                             the log's contact_step (in cursor units; -1 if none or no log), the log's flags (0 without a log), due[q][g], 0
 *        ep_f64[q][g][0..1] = the log's min_clearance (+inf without a log), 0
 *      so that the episode's log rows are [row_end - steps_driven, row_end) of the slot's rows;
 *   2. increments served[q];
 *   3. if served[q] < generations, puts the slot's per-agent state back to "first step of a fresh batch" -- state = start_state, applied = 0,
 *      traj_idx = target_ind = start_idx, cut_len = 0 (MPCX_STOP_SPEED: prev_len = 0 too), u_sol = 0, iters = 0, steps_driven = 0; with a log
 *      goal_step = contact_step = -1, flags = 0, min_clearance = +inf, while the cursor `steps` keeps counting: a slot's log rows are its
 *      vehicles' rows one after the other -- and hands it to the admission gate: entered_step = -1, wait = max(0, due[q][served[q]] - clock).
 *      The next vehicle asks to enter in step max(next step, its due step) and goes through the gate like any scheduled agent: a reset slot
 *      is a waiting agent in exactly the state admission defines (done[q] = 1, own row absent, wait[q] >= 0);
 *   4. otherwise the slot is finished: it stays departed and is never touched again.
 * x_sol, xref, xbar, reaches_end, status, kkt, hit_idx and hit_xy are pure outputs: they stay as the last vehicle left them until the new
 * vehicle's first step overwrites them, and nothing reads them for a waiting agent.  steps_driven == arrived_step - entered_step + 1 in every
 * record, because an agent in the scene drives every step -- except for a slot found arrived when respawn is switched on (an agent that
 * arrived earlier, or an unscheduled one retired by the caller's goal test before the first step): it counts as arriving in that step.
 * due[q][0] is recorded only: the FIRST vehicle of a slot enters as the caller's mpcx_admit::wait says.
 * Everything that changes is device memory, so a replayed graph respawns like a plain run.  The struct travels beside the descriptor (no
 * other struct changes size); the cached graph's key covers it by value.  respawn = NULL or an all-zero struct: mpcx_closed_loop_run_admit
 * itself -- the same launches with the same arguments.  MPCX_E_INVALID ("respawn: ...") before anything is launched, whatever n_steps is:
 * respawn without admission (which in turn needs a scene and retirement, and so refuses MPCX_SHARD_AGENTS and more than one linearisation
 * pass); generations < 1; one of the six pointers NULL.  The step order becomes admit -> ... -> record -> retire -> respawn.
 * Works with scripted traffic, the run log, both stop modes and use_graph. */
typedef struct {
    int32_t generations;          /* G >= 1: vehicles per slot */
    int32_t reserved;
    const double  *start_state;   /* P,4 */
    const int32_t *start_idx;     /* P */
    const int32_t *due;           /* P,G: step index at which vehicle g of slot q asks to enter; [q][0] is recorded only */
    int32_t *served;              /* P, zero-initialised */
    int32_t *ep_i32;              /* P,G,8 */
    double  *ep_f64;              /* P,G,2 */
} mpcx_respawn;
int32_t mpcx_closed_loop_run_respawn(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                     const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                     const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                     const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                     int32_t n_steps, int32_t use_graph);
/* one step's respawn as a stage of its own (what mpcx_closed_loop_run_respawn enqueues at the end of a step): the buffers are the closed
 * loop's; prev_len is mpcx_closed_loop_opts::prev_len (NULL in MPCX_STOP_CUT), obs_skip names the agents' own rows among the n_obs_pool rows
 * of the pool, log may be NULL.  The stage reads retire->done and admit->clock and writes retire->steps_driven, admit->wait and
 * admit->entered_step.  u_sol is P x 2 x T doubles, T that of mpcx_set_mpc_params. */
int32_t mpcx_respawn_step_batch(mpcx_ctx *ctx, int32_t P, double *state /*P,4*/, double *applied /*P,2*/, double *u_sol /*P,2,T*/,
                                int32_t *traj_idx /*P*/, int32_t *target_ind /*P*/, int32_t *cut_len /*P*/, int32_t *iters /*P*/,
                                int32_t *prev_len /*P or NULL*/, const int32_t *obs_skip /*P*/, int32_t n_obs_pool,
                                const mpcx_run_log *log /*or NULL*/, const mpcx_retire *retire, const mpcx_admit *admit,
                                const mpcx_respawn *respawn);

/* ---- routes: every vehicle of a slot takes its own route from its own start pose.  With respawn alone a slot is bound to one route and one
 * start pose for the whole run; with routes vehicle g of slot q drives route route_of[q][g] (an index into the n_routes-word tables route_off /
 * route_len, which name runs of the descriptor's path tables -- every path table is indexed by absolute path point, so a route is two words)
 * from start_state[q][g] and path index start_idx[q][g].  respawn_route_kernel (csrc/mpcx_route.hip; the rule is csrc/mpcx_route_core.h)
 * is launched IN PLACE OF respawn_kernel: a step has the launches of a respawn step.  For agent q, in this order:
 *   1. g = served[q], read before anything else;
 *   2. the respawn rule itself (csrc/mpcx_respawn_core.h, called, not restated);
 *   3. if the agent arrived: ep_i32[q][g][7] = route_of[q][g] -- the reserved word of the episode record now names the episode's route;
 *   4. if the slot was reset (served[q] < generations now), with g' = g + 1 and r = route_of[q][g'], what the reset wrote is overwritten:
 *      state[q] = start_state[q][g'], traj_idx[q] = target_ind[q] = start_idx[q][g'], path_off[q] = route_off[r], path_len[q] = route_len[r];
 *   5. a DEFECTIVE next vehicle -- r outside [0, n_routes) or start_idx[q][g'] outside [0, route_len[r]) -- is never driven: the slot is left
 *      with wait = -1, entered_step = -1, done set and its row absent, so it neither drives nor waits and never arrives again; path_off and
 *      path_len are not touched.
 * mpcx_respawn::start_state / start_idx are still required and still what the plain reset writes; with routes nothing reads them afterwards.
 * Vehicle 0 of a slot is the caller's: path_off, path_len, state, traj_idx and target_ind as the batch stands when the run starts.
 * path_off and path_len MUST be the descriptor's own (the stages read them afresh every step; here they become writable).  Every access is
 * to words of agent q plus the read-only route tables: the outcome does not depend on the order of the lanes.  Everything that changes is
 * device memory, so a replayed graph routes like a plain run.  The struct travels beside the descriptor (no other struct changes size); the
 * cached graph's key covers it by value.  routes = NULL or an all-zero struct: mpcx_closed_loop_run_respawn itself -- the same launches with
 * the same arguments.  MPCX_E_INVALID ("routes: ...") before anything is launched, whatever n_steps is: routes without respawn; one of the
 * seven pointers NULL; n_routes < 1; path_off / path_len that are not the descriptor's; a route_len[r] below 1 or above the conflict
 * search's capacity (mpcx_interaction_params.max_path_len as mpcx_interaction_batch rounds it).  route_off and route_len are read back once
 * per call, as the row maps of scripted traffic are; the per-vehicle tables are not: the kernel's own test (5.) covers them.  That a route's
 * run lies inside the path tables is the caller's word, as path_off / path_len are. */
typedef struct {
    int32_t n_routes;             /* R >= 1 */
    int32_t reserved;
    const int32_t *route_off;     /* R: first path point of route r in the descriptor's path tables */
    const int32_t *route_len;     /* R: its length in points */
    const int32_t *route_of;      /* P,G: the route of vehicle g of slot q */
    const double  *start_state;   /* P,G,4 */
    const int32_t *start_idx;     /* P,G */
    int32_t *path_off;            /* P: mpcx_closed_loop::path_off itself */
    int32_t *path_len;            /* P: mpcx_closed_loop::path_len itself */
} mpcx_routes;
int32_t mpcx_closed_loop_run_routes(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                    const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                    const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                    const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                    const mpcx_routes *routes /*or NULL*/, int32_t n_steps, int32_t use_graph);
/* one step's routed respawn as a stage of its own: mpcx_respawn_step_batch with the routes struct (NULL or all-zero: that call itself).
 * routes->path_off / path_len are the P words the stage may write; max_path_len bounds route_len as the closed loop's check does (0: no
 * upper bound is checked). */
int32_t mpcx_respawn_step_batch_routes(mpcx_ctx *ctx, int32_t P, double *state /*P,4*/, double *applied /*P,2*/, double *u_sol /*P,2,T*/,
                                       int32_t *traj_idx /*P*/, int32_t *target_ind /*P*/, int32_t *cut_len /*P*/, int32_t *iters /*P*/,
                                       int32_t *prev_len /*P or NULL*/, const int32_t *obs_skip /*P*/, int32_t n_obs_pool,
                                       const mpcx_run_log *log /*or NULL*/, const mpcx_retire *retire, const mpcx_admit *admit,
                                       const mpcx_respawn *respawn, const mpcx_routes *routes /*or NULL*/, int32_t max_path_len);
/* the per-movement table of a routed run, reduced on the device: per instance b (A consecutive slots of the P = B A) and route r, over the
 * FINISHED episodes (g < served[q]) whose word 7 is r,
 *   out_i64[b][r][0..3] = the number of episodes, the number with a contact (contact_step >= 0), the sum of entered - due, the sum of
 *                         steps_driven
 *   out_f64[b][r]       = the minimum of min_clearance (+inf if there are none; a NaN is skipped)
 * Integer sums and a minimum only: the table is exact whatever the mapping of records to lanes.  One wavefront per instance (csrc/
 * mpcx_route.hip, summary_kernel).  Episodes whose word 7 lies outside [0, R) are in no row.  All pointers are device pointers; enqueued on
 * the context's stream.  MPCX_E_INVALID: a negative size, A < 1 with P > 0, P not a multiple of A, G < 1, R < 1, a NULL pointer. */
int32_t mpcx_episode_summary(mpcx_ctx *ctx, int32_t P, int32_t A, int32_t G, int32_t R, const int32_t *served /*P*/,
                             const int32_t *ep_i32 /*P,G,8*/, const double *ep_f64 /*P,G,2*/, int64_t *out_i64 /*B,R,4*/,
                             double *out_f64 /*B,R*/);

/* ---- right of way: who yields to whom.  The reference's other cars are scripted and never yield, and its ego yields to all of them; in a loop
 * of many egos that rule makes everybody yield to everybody, and cars that meet at the crossing wait for each other for ever.  Precedence is
 * an opt-in rule beside mpcx_scene that breaks the mutual wait.  One int32 word per pool row, prec[n_rows], caller-owned DEVICE memory; a
 * SMALLER word goes first.  For a driving agent q with own row o = obs_skip[q] and a present row r != o of its window:
 *   prec[r] <= prec[o]   q sees r as it does without precedence, through its prediction (equal words: the reference's mutual yield);
 *   prec[r] >  prec[o]   r yields to q, and q sees r STANDING: every frame of r's prediction is the two disc centres of r's current pose.
 * Absent rows stay invisible.  A scripted actor's row keeps the word the caller gave it: zero means everybody (whose word is >= 0) sees it
 * moving.  The defining property: for every driving agent a step with precedence equals a step of the scene loop in which every yielding
 * row (x, y, v, yaw, a, steer) of its obstacle list is replaced by (x, y, 0, yaw, 0, 0), relative order kept -- the rollout of such a row
 * reproduces its pose exactly, so this holds bit for bit.  A yielding car is thus still an obstacle where it stands (a car with precedence
 * does not drive into one that is already in its way); what it no longer does is claim the road ahead of it.  With all words equal the run
 * is the scene run bit for bit.  The run log's clearance and contact (true clearance), the admission gate, retirement, respawn and routes
 * do not change.
 * stand[n_rows][4] is caller-owned device scratch: predict_kernel's STAND instantiation stores every predicted row's standing record there,
 * and interaction_kernel's PREC instantiation loads a yielding row's candidates from it instead of from the prediction.
 * mode:
 *   MPCX_PRECEDENCE_FIXED   the loop never writes prec: the caller's words hold.
 *   MPCX_PRECEDENCE_ENTRY   first come, first served; needs admission.  Right after a step's admission stage one more launch
 *                           (precedence_stamp_kernel, csrc/mpcx_precedence.hip; the rule is csrc/mpcx_precedence_core.h) writes, for every
 *                           agent with entered_step[q] >= 0, prec[obs_skip[q]] = entered_step[q] * 64 + (obs_skip[q] - obs_off[q]): ties
 *                           go to the lower window offset (a scene window holds at most 64 rows).  The words of waiting agents and of
 *                           other rows are not touched; a respawned vehicle gets its word in the step that admits it and so queues behind
 *                           everybody already in the scene.  entered_step * 64 wraps from step 2^25 on: the caller's limit.
 * The struct travels beside the descriptor (no other struct changes size); the cached graph's key covers it by value.  precedence = NULL
 * or an all-zero struct: mpcx_closed_loop_run_routes itself -- the same launches with the same arguments.  MPCX_E_INVALID
 * ("precedence: ...") before anything is launched, whatever n_steps is: an unknown mode; precedence without a scene (which in turn needs
 * retirement and refuses MPCX_SHARD_AGENTS and more than one linearisation pass); prec or stand NULL; n_rows that is not the pool's row
 * count; MPCX_PRECEDENCE_ENTRY without admission.  Works with scripted traffic, the run log, both stop modes and use_graph. */
enum { MPCX_PRECEDENCE_FIXED = 1, MPCX_PRECEDENCE_ENTRY = 2 };
typedef struct {
    int32_t *prec;       /* n_rows, caller-owned: the precedence word of every pool row, a smaller word goes first */
    double *stand;       /* n_rows x 4, caller-owned scratch: the standing records */
    int32_t n_rows;      /* rows of the pool: mpcx_scene::n_rows */
    int32_t mode;        /* MPCX_PRECEDENCE_* */
} mpcx_precedence;
int32_t mpcx_closed_loop_run_precedence(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                        const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                        const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                        const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                        const mpcx_routes *routes /*or NULL*/, const mpcx_precedence *precedence /*or NULL*/,
                                        int32_t n_steps, int32_t use_graph);
/* one step's admission followed by the entry-order stamp, as a stage of its own (what mpcx_closed_loop_run_precedence enqueues at the head
 * of a step): mpcx_admit_step_batch with the precedence struct (NULL or all-zero: that call itself; MPCX_PRECEDENCE_FIXED: that call after
 * the struct's check).  The scene the struct is checked against is `absent` over the n_obs_pool rows. */
int32_t mpcx_admit_step_batch_precedence(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state /*P,4*/,
                                         const int32_t *obs_off /*P*/, const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P*/,
                                         int32_t *done /*P*/, int32_t n_obs_pool, int32_t *absent /*NOBS*/,
                                         int32_t n_actors, const mpcx_traffic_actor *actors /*n_actors*/, const double *actor_state /*n_actors,4*/,
                                         const double *tape /*rows,6 or NULL*/, int64_t tape_rows, const int32_t *actor_row /*n_actors*/,
                                         const mpcx_admit *admit, const mpcx_precedence *precedence /*or NULL*/);

/* ---- traffic signals: agents are held at stop lines.  A signalised crossing separates conflicting movements in time, and a car that must
 * wait does so at a stop line outside the crossing.  The reference holds an ego by ending its path in front of a conflict
 * (tmp_trajectory = trajectory_full[:cutoff_idx]); a red light is a conflict at a known point of the agent's own path, so the rule is one
 * small stage directly behind the conflict search (signal_kernel, csrc/mpcx_signal.hip; the rule is csrc/mpcx_signal_core.h) that
 * shortens cut_len -- the cut length, or the stop index in MPCX_STOP_SPEED -- and touches nothing else.
 * Stop lines are a property of PATH POINTS, two int32 tables parallel to the descriptor's path tables: path_stop[i] is the route-local
 * index s of the next stop-line point at or after point i (-1: none ahead), path_group[i] that line's signal group (0 .. n_groups - 1,
 * n_groups <= MPCX_SIGNAL_GROUPS_MAX = 16).  Plans -- a table, so that a sweep of signal timings runs as one batch --: plan_cycle[n_plans]
 * (steps, >= 1), plan_amber[n_plans] (steps, >= 0), plan_green[n_plans][n_groups][2] = (green_from in [0, cycle), green_len >= 0, with
 * green_len + amber <= cycle), plan_of[P] the plan of agent q.  The clock is one word per agent, tick[P]: agent q's lane reads t = tick[q]
 * reduced into [0, cycle) and writes back t + 1 wrapped at cycle, in every step whether the agent drives or not; an offset is the initial
 * tick.  Light of group g at t: u = t - green_from (+ cycle if negative); GREEN if u < green_len, AMBER if u < green_len + amber, else RED.
 * Per agent q after the tick: done[q] (retirement) -> held[q] = 0 and nothing else.  With i = path_off[q] + traj_idx[q] (traj_idx as this
 * step's conflict search left it), s = path_stop[i], g = path_group[i] the agent is FREE (held[q] = 0) with no line ahead (s < 0), on or
 * past the line (traj_idx[q] >= s) or with a defective entry (i outside [0, n_points), g or plan_of[q] out of range, s >= path_len[q]).
 * Otherwise GREEN: free; RED: held[q] = 1; AMBER: held[q] = 2 if held[q] was nonzero already or if the car can stop,
 * (s - traj_idx[q]) * dl >= v * v / (2 * brake) with v = state[q][2], else free.  held is in-out (the decision in amber is sticky) and
 * zero-initialised by the caller.  A held agent gets cut_len[q] = min(cut_len[q], s): its path ends on the point before the line.
 * hit_idx and hit_xy stay the conflict search's.  The defining property: a step with signals equals the step without them in which, for
 * every held agent, the cut length / stop index the conflict search produced is replaced by its minimum with s before the window stage.
 * (The conflict search has filed the agent in the QP work queue under a key computed from the cut before this stage: that affects the
 * queue order only, never a result.  In speed mode a stop index equal to 999 reads as "no stop", as in the reference.)
 * The struct travels beside the descriptor (no other struct changes size); the cached graph's key covers it by value.  signals = NULL or
 * an all-zero struct: mpcx_closed_loop_run_precedence itself -- the same launches with the same arguments.  MPCX_E_INVALID
 * ("signals: ...") before anything is launched, whatever n_steps is: a NULL pointer; n_groups outside 1..16; n_plans < 1 or n_points < 1;
 * brake not finite or not positive; a plan with cycle < 1, amber < 0, green_from outside [0, cycle), green_len < 0 or green_len + amber >
 * cycle (the three plan tables are read back once per call; the per-agent and per-point tables are not -- the kernel's own tests cover
 * them); the agent-sharded layout; more than one linearisation pass.  Works with scripted traffic, the run log, retirement, scene,
 * admission, respawn, routes, precedence, both stop modes and use_graph, and needs none of them. */
#define MPCX_SIGNAL_GROUPS_MAX 16
typedef struct {
    const int32_t *path_stop;    /* n_points: route-local index of the next stop line at or after this path point, -1 = none ahead */
    const int32_t *path_group;   /* n_points: that line's signal group */
    const int32_t *plan_cycle;   /* n_plans: cycle length in steps, >= 1 */
    const int32_t *plan_amber;   /* n_plans: amber length in steps, >= 0 */
    const int32_t *plan_green;   /* n_plans x n_groups x 2: (green_from, green_len) */
    const int32_t *plan_of;      /* P: the plan of agent q */
    int32_t *tick;               /* P, caller-owned, in-out: the agent's clock */
    int32_t *held;               /* P, caller-owned, in-out, zero-initialised: 0 free, 1 held at red, 2 held at amber */
    double brake;                /* the deceleration (> 0, m/s^2) an agent is trusted to stop with in amber */
    int32_t n_points, n_plans, n_groups, reserved;   /* reserved: 0 */
} mpcx_signals;
int32_t mpcx_closed_loop_run_signals(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                     const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                     const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                     const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                     const mpcx_routes *routes /*or NULL*/, const mpcx_precedence *precedence /*or NULL*/,
                                     const mpcx_signals *signals /*or NULL*/, int32_t n_steps, int32_t use_graph);
/* one step's signal stage alone (what mpcx_closed_loop_run_signals enqueues between the conflict search and the window stage): cut_len is
 * the conflict search's output of this step, in-out; done: mpcx_retire::done or NULL.  The struct is checked as above. */
int32_t mpcx_signal_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const int32_t *path_off /*P*/,
                               const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *cut_len /*P*/,
                               const int32_t *done /*P or NULL*/, const mpcx_signals *signals);

/* ---- vehicle-actuated signals: a controller per junction decides the lights from who is waiting.  mpcx_signals with a fixed plan gives an
 * empty approach its green while the loaded one queues; the controller of a real junction holds a phase at least its minimum green,
 * extends it while its own detectors are occupied, ends it when they have been empty for a gap, or at a maximum -- but only if somebody
 * else is waiting -- and skips phases nobody calls.  One launch (actuated_signal_kernel, csrc/mpcx_actuated.hip; the rule is
 * csrc/mpcx_actuated_core.h) takes the place of signal_kernel: a step with actuation has the launches of a step with signals.  It replaces
 * the SOURCE OF THE LIGHT and nothing else: the hold at the line is the rule of mpcx_signals, word for word.
 * A junction is n_per consecutive agents: junction j owns agents [j n_per, (j + 1) n_per), n_per n_junctions = P.  A controller (one timing
 * set) has n_phases phases (1 .. MPCX_ACTUATION_PHASES_MAX = 8); a table of n_ctrl controllers runs a sweep as one batch:
 * phase_groups[n_ctrl][n_phases] the bitmask of the signal groups green in the phase, phase_time[n_ctrl][n_phases][3] = (min_green,
 * max_green, gap) in steps, ctrl_time[n_ctrl][3] = (amber, all_red in steps, detect in path points), ctrl_of[n_junctions] the controller of
 * junction j.  jstate[n_junctions][4] = (phase, stage, timer, idle), stage 0 GREEN, 1 AMBER, 2 ALL_RED, caller-owned device memory, in-out,
 * zero-initialised; lights[n_junctions] (out): 2 bits per group, MPCX_SIGNAL_GREEN / AMBER / RED; calls[n_junctions] (out): bit g set when
 * group g is called this step.
 * Per junction and step: (1) read (p, stage, timer, idle); a defective word -- p outside [0, n_phases), stage outside 0..2, a negative
 * timer or idle -- counts as (0, GREEN, 0, 0); a junction whose ctrl_of is out of range has no controller: its agents are free (held = 0),
 * its jstate is left alone, lights = calls = 0.  (2) the lights of this step from the state as read: GREEN -- the groups of
 * phase_groups[p] green, all others red; AMBER -- those groups amber, all others red; ALL_RED -- all red.  (3) calls: bit g is set if some
 * agent q of the junction is not done (done NULL or done[q] == 0), stands on a valid point in front of its line (i = path_off[q] +
 * traj_idx[q] in [0, n_points), s = path_stop[i] with 0 <= s < path_len[q], traj_idx[q] < s, g = path_group[i] in [0, n_groups)) and inside
 * the detector, s - traj_idx[q] <= detect.  (4) advance, with D_k = (calls & phase_groups[k]) != 0 and other = some k != p has D_k.
 * GREEN: timer' = min(timer + 1, max_green), idle' = D_p ? 0 : min(idle + 1, gap); the phase ends if other and timer' >= min_green and
 * (idle' >= gap or timer' >= max_green), else it rests in green -- a phase nobody contests never ends.  AMBER: timer' = timer + 1, ends at
 * timer' >= amber; ALL_RED the same with all_red.  Leaving goes GREEN -> AMBER -> ALL_RED -> GREEN of the next phase with timer = idle = 0
 * on entry; a stage of length 0 is passed through in the same step.  The next phase is the first k in ring order p + 1, p + 2, ... (mod
 * n_phases, p excluded) with D_k by this step's calls, (p + 1) % n_phases if there is none.  (5) every agent of the junction goes through
 * steps 2 - 5 of the signal rule with the light of its group taken from lights[j].
 * With actuation mpcx_signals supplies path_stop, path_group, held, brake, n_points and n_groups; its plan_cycle, plan_amber, plan_green,
 * plan_of and tick must be NULL and n_plans 0.  actuation = NULL or an all-zero struct: mpcx_closed_loop_run_signals itself -- the same
 * launches with the same arguments.  No other struct changes size; the cached graph's key covers the struct by value.  MPCX_E_INVALID
 * ("actuation: ...") before anything is launched, whatever n_steps is: a NULL pointer; actuation without signals, or signals that also
 * carry a fixed plan; n_per < 1 or n_per n_junctions != P; n_phases outside 1..8; n_ctrl < 1; reserved != 0; a phase mask that is zero or
 * has bits at or above n_groups; min_green < 0, max_green < 1, min_green > max_green, gap < 1; amber < 0, all_red < 0, detect < 1 (the three
 * controller tables are read back once per call; the per-junction, per-agent and per-point words are not -- a bad word is never a GPU
 * fault); signals' own refusals of n_groups, n_points and brake; the agent-sharded layout; more than one linearisation pass. */
#define MPCX_ACTUATION_PHASES_MAX 8
#define MPCX_STAGE_GREEN 0
#define MPCX_STAGE_AMBER 1
#define MPCX_STAGE_ALL_RED 2
typedef struct {
    const int32_t *phase_groups; /* n_ctrl x n_phases: bitmask of the signal groups green in the phase */
    const int32_t *phase_time;   /* n_ctrl x n_phases x 3: (min_green, max_green, gap), steps */
    const int32_t *ctrl_time;    /* n_ctrl x 3: (amber, all_red) in steps, detect in path points */
    const int32_t *ctrl_of;      /* n_junctions: the controller of junction j */
    int32_t *jstate;             /* n_junctions x 4, caller-owned, in-out, zero-initialised: (phase, stage, timer, idle) */
    int32_t *lights;             /* n_junctions, out: 2 bits per group */
    int32_t *calls;              /* n_junctions, out: bit g = group g is called this step */
    int32_t n_per, n_junctions, n_phases, n_ctrl, reserved;      /* reserved: 0 */
} mpcx_actuation;
int32_t mpcx_closed_loop_run_actuated(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                      const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                      const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                      const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                      const mpcx_routes *routes /*or NULL*/, const mpcx_precedence *precedence /*or NULL*/,
                                      const mpcx_signals *signals /*or NULL*/, const mpcx_actuation *actuation /*or NULL*/, int32_t n_steps,
                                      int32_t use_graph);
/* one step's actuated signal stage alone (what mpcx_closed_loop_run_actuated enqueues between the conflict search and the window stage);
 * the arguments of mpcx_signal_step_batch plus the controller.  Both structs are checked as above. */
int32_t mpcx_actuated_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const int32_t *path_off /*P*/,
                                 const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *cut_len /*P*/,
                                 const int32_t *done /*P or NULL*/, const mpcx_signals *signals, const mpcx_actuation *actuation);

/* ---- signal-aware approach speed: agents are advised ahead of a red light.  In MPCX_STOP_SPEED a hold only zeroes the speed reference
 * from the stop line on; the path stays whole and the position reference keeps pulling the car forward, so it reaches its line at speed,
 * brakes late and creeps over.  The plan is a table in device memory: an agent can know when its light turns green.  One launch per step
 * (advise_kernel, csrc/mpcx_advise.hip; the rule is csrc/mpcx_advise_core.h) between the window stage and the QP caps row 2 of the agent's
 * xref -- the speed reference over the window -- at the speed with which it reaches its line as the light turns green, and touches nothing
 * else.  The hold of mpcx_signals stays as it is, the safety net behind the advice; a held agent IS advised.
 * For agent q, with traj_idx, cut_len, tick and held as the signal stage of this step left them:  (1) NO ADVICE, advised[q] = 0.0 and xref
 * untouched: done[q] != 0; plan_of[q] out of range or cycle < 1; any "free" condition of the hold -- with i = path_off[q] + traj_idx[q]: i
 * outside [0, n_points), s = path_stop[i] < 0, traj_idx[q] >= s, s >= path_len[q], the group out of range --; cut_len[q] < s (a conflict
 * stops the agent before its line); d > reach with d = (double)(s - traj_idx[q]) * dl.  (2) t0 = tick[q] - 1 (+ cycle if negative): the
 * clock value the signal stage used this step.  (3) k_c = ceil(d / (v_cruise * dt)), an integer clamped to 2^30, dt the context's MPC
 * time step: the earliest arrival; u = (t0 + k_c - green_from) mod cycle, non-negative; u < green_len: arrival on green at cruise speed, no
 * advice.  (4) else w = cycle - u, k_t = k_c + w + lead, v = d / ((double)k_t * dt), advised[q] = max(v, v_min).  (5) every entry of row 2
 * of agent q's xref (T + 1 doubles at xref + (4 q + 2)(T + 1)) becomes fmin(entry, advised[q]): the zeros of the stop profile stay zero.
 * The result is bit-identical between a host build of the rule and the device and does not depend on the order of the lanes.
 * advice = NULL or an all-zero struct: mpcx_closed_loop_run_actuated itself -- the same launches with the same arguments.  No other struct
 * changes size; the cached graph's key covers the struct by value.  MPCX_E_INVALID ("advice: ...") before anything is launched, whatever
 * n_steps is: advised NULL; n_rows != P; v_cruise, v_min or reach not finite or not positive; v_min > v_cruise; lead < 0; no signals, or
 * signals without a fixed plan; actuation on (a controller decides the lights step by step: there is no plan to look ahead into); a stop
 * mode other than MPCX_STOP_SPEED (in cut mode the speed reference is 0 and the stage would silently do nothing); the signals' own
 * refusals.  The struct has no padding: two int32 close its 40 bytes. */
typedef struct {
    double *advised;             /* n_rows = P, caller-owned, out: the speed advised to agent q in the last step, 0.0 = none */
    double v_cruise;             /* the speed the earliest arrival is computed with (> 0, m/s) */
    double v_min;                /* advice is never below this (> 0, <= v_cruise, m/s) */
    double reach;                /* only agents within this distance of their line are advised (> 0, m) */
    int32_t lead, n_rows;        /* lead: steps of margin added to the wait (>= 0); n_rows: P */
} mpcx_advice;
/* the widest entry point: mpcx_closed_loop_run_actuated with the advice stage */
int32_t mpcx_closed_loop_run_advised(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                     const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                     const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                     const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                     const mpcx_routes *routes /*or NULL*/, const mpcx_precedence *precedence /*or NULL*/,
                                     const mpcx_signals *signals /*or NULL*/, const mpcx_actuation *actuation /*or NULL*/,
                                     const mpcx_advice *advice /*or NULL*/, int32_t n_steps, int32_t use_graph);
/* one step's advice stage alone (what mpcx_closed_loop_run_advised enqueues between the window stage and the QP): xref is the window
 * stage's output of this step (P x 4 x (T + 1), T the context's horizon), row 2 of it in-out; done: mpcx_retire::done or NULL.  Both
 * structs are checked as above (the caller vouches for the stop mode: xref is that of mpcx_mpc_prepare_batch_stop). */
int32_t mpcx_advise_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const int32_t *path_off /*P*/, const int32_t *path_len /*P*/,
                               const int32_t *traj_idx /*P*/, const int32_t *cut_len /*P*/, const int32_t *done /*P or NULL*/,
                               const mpcx_signals *signals, const mpcx_advice *advice, double *xref /*P,4,T+1*/);

/* ---- shared plans: a connected agent is predicted from its last MPC solution.  The prediction stage is the reference's
 * MovingObstaclesPrediction: the controls applied in the last step, held for pred_steps frames -- right for a scripted car, which has no
 * plan, wrong for an MPC agent, whose plan of one step ago (u_sol, still resident when the prediction runs) already holds its braking in
 * front of a cut path, a stop line or an advised speed.  One launch per step (intent_kernel, csrc/mpcx_intent.hip; the rule is
 * csrc/mpcx_intent_core.h) between the prediction and the conflict search overwrites the frames of a sharing agent's OWN pool row
 * r = obs_skip[q] with its plan re-rolled through the prediction's model, and touches no other row.
 * For agent q: row r is left as the prediction stage wrote it and frames[q] = 0 if share[q] == 0; done[q] != 0; absent[r] != 0;
 * status[q] != MPCX_QP_OPTIMAL (the plant applied max_decel and zeroed the warm start: the constant prediction is then the truth).
 * Otherwise, from (x, y, v, yaw) = state[q], frame k = 0 .. pred_steps - 1 takes acc = u_sol[q][0][j], steer = u_sol[q][1][j],
 * j = min(k + 1, T - 1) (column 0 was applied in the step just taken; beyond the plan the last column is held), and the prediction's
 * updates in its order: x += (v cos yaw) dt; y += (v sin yaw) dt; v += acc dt; yaw += ((v / L) tan steer) dt (v is not clamped); then
 * the two disc centres of the pose; frames[q] = pred_steps.  Bit for bit on the device: a plan whose columns j >= 1 all equal the
 * applied controls, and any plan with T = 1, leave the prediction stage's own frames.
 * intent = NULL or an all-zero struct: mpcx_closed_loop_run_advised itself -- the same launches with the same arguments.  No other struct
 * changes size; the cached graph's key covers the struct by value.  A run with the stage on does not take step fusion.  MPCX_E_INVALID
 * ("intent: ...") before anything is launched, whatever n_steps is: share or frames NULL; n_rows != P; no pool or no obs_skip; an
 * obs_skip[q] outside the pool (read back once); exchange == MPCX_SHARD_AGENTS (the other ranks' rows arrive without their plans).
 * The struct has no padding: two int32 close its 24 bytes. */
typedef struct {
    const int32_t *share;        /* n_rows = P, caller-owned: nonzero = agent q shares its plan */
    int32_t *frames;             /* n_rows = P, caller-owned, out: frames of agent q's row taken from its plan in the last step (pred_steps or 0) */
    int32_t n_rows;              /* P */
    int32_t reserved;            /* 0 */
} mpcx_intent;
/* the widest entry point: mpcx_closed_loop_run_advised with the shared-plans stage */
int32_t mpcx_closed_loop_run_intent(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                    const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                    const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                    const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                    const mpcx_routes *routes /*or NULL*/, const mpcx_precedence *precedence /*or NULL*/,
                                    const mpcx_signals *signals /*or NULL*/, const mpcx_actuation *actuation /*or NULL*/,
                                    const mpcx_advice *advice /*or NULL*/, const mpcx_intent *intent /*or NULL*/, int32_t n_steps,
                                    int32_t use_graph);
/* mpcx_interaction_batch with the shared-plans stage between its prediction and its conflict search: u_sol (P x 2 x T, T the context's
 * horizon) and status (P) are the previous solve's; done (P) and absent (n_obs_pool) may be NULL and are read by the stage alone.  The
 * struct is checked as above (an all-zero or NULL struct is refused here: the call exists for the stage); obs_skip is required. */
int32_t mpcx_interaction_batch_intent(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                                      const double *state /*P,4*/, const double *path_xyyaw, const double *path_cs,
                                      const int32_t *path_off /*P*/, const int32_t *path_len /*P*/, const int32_t *prev_cut_len /*P or NULL*/,
                                      int32_t n_obs_pool, const double *obs6 /*NOBS,6*/, const int32_t *obs_off /*P*/,
                                      const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P*/,
                                      int32_t *traj_idx /*P in-out*/, int32_t *hit_idx /*P*/, double *hit_xy /*P,2*/, int32_t *cut_len /*P*/,
                                      const double *u_sol /*P,2,T*/, const int32_t *status /*P*/, const int32_t *done /*P or NULL*/,
                                      const int32_t *absent /*NOBS or NULL*/, const mpcx_intent *intent);

/* ---- crossing reservations: a manager per junction admits only compatible movements.  Signals, fixed or actuated, separate PHASES and
 * leave the turns inside a phase to the conflict search; an unsignalised crossing of connected vehicles is run by a manager that admits a
 * car only if its MOVEMENT conflicts with no movement that holds the crossing, first come, first served, while the others wait at their
 * stop lines.  One launch (reserve_kernel, csrc/mpcx_reserve.hip; the rule is csrc/mpcx_reserve_core.h) takes the place of signal_kernel /
 * actuated_signal_kernel: a third source of "may I enter" beside the fixed plan and the controller; the hold at the line is the rule of
 * mpcx_signals, word for word, with GREEN for an agent that holds a reservation and RED for one that does not.  No amber.
 * The movement of an agent is the signal group of its stop line (path_group).  A junction is n_per consecutive agents, n_per <= 64:
 * junction j owns agents [j n_per, (j + 1) n_per), n_per n_junctions = P.  Tables: path_exit[n_points] the route-local index e at which a
 * vehicle on this point has left the crossing, -1 if no crossing lies ahead or under the point; conflict[n_groups], bit h of word g set
 * when movements g and h may not hold the crossing together (symmetric, no diagonal); lane[n_groups], bit h of word g set when they queue
 * in the same approach lane (symmetric, bit g of word g set); mgr_time[n_mgr][2] = (detect in path points, patience in steps);
 * mgr_of[n_junctions] the manager of junction j -- a table of managers runs a sweep as one batch.  State, caller-owned device memory:
 * grant[P] in-out, zero-initialised (0, or 1 = the agent holds a reservation); since[P] in-out, initialised to -1 (the clock value of the
 * agent's first request); clock[n_junctions] in-out, zero-initialised; occupied[n_junctions] out (the movements that hold the crossing);
 * queued[n_junctions] out (the requesters denied this step).
 * Per junction and step: (1) t = clock[j], a negative word counts as 0; clock[j] = t + 1.  A junction whose mgr_of is out of range has no
 * manager: its agents are free (held = 0), grant, since and clock are left alone, occupied = queued = 0.  (2) every agent q, with ti =
 * traj_idx[q] as this step's conflict search left it, i = path_off[q] + ti, s = path_stop[i], g = path_group[i], e = path_exit[i]: OUT
 * (grant = 0, since = -1) if done[q] != 0, i outside [0, n_points), e < 0, e > path_len[q], ti >= e, g outside [0, n_groups), or ti < s
 * with s >= path_len[q]; INSIDE (grant = 1, it occupies g whatever grant was; since is left alone) if not OUT and (s < 0 or ti >= s);
 * otherwise APPROACH: with grant != 0 it occupies g (a grant is never revoked; grant and since are left alone), without one and with
 * s - ti <= detect it REQUESTS, since = since >= 0 ? since : t, otherwise since = -1.  (3) occ = OR of 1 << g over the occupying agents.
 * (4) the requesters in ascending order of (since, min(s - ti, 65535), index within the junction), from ahead = blocked = 0: a requester of
 * movement g is granted (grant = 1, occ |= 1 << g) if (conflict[g] & (occ | blocked)) == 0 and (lane[g] & ahead) == 0; otherwise it is
 * denied, ahead |= 1 << g, and if it is aged, (int64) t - since >= patience, also blocked |= 1 << g.  patience = 0 is strict first come,
 * first served; a large patience lets later compatible cars pass a waiting one; any finite patience rules out starvation.  (5)
 * occupied[j] = occ, queued[j] = the number denied.  (6) every agent goes through steps 2 - 5 of the signal rule: an APPROACH agent
 * without a grant, requesting or not, gets held = 1 and cut_len = min(cut_len, s); everybody else is free.
 * In MPCX_STOP_SPEED the soft stop can roll a held car over its line; it then counts as INSIDE and occupies its movement.
 * With reservations mpcx_signals supplies path_stop, path_group, held, brake, n_points and n_groups; its plan_cycle, plan_amber,
 * plan_green, plan_of and tick must be NULL and n_plans 0.  reservation = NULL or an all-zero struct: mpcx_closed_loop_run_intent itself
 * -- the same launches with the same arguments.  No other struct changes size; the cached graph's key covers the struct by value (it has
 * no padding: four int32 close its 96 bytes).  MPCX_E_INVALID ("reservation: ...") before anything is launched, whatever n_steps is: a
 * NULL pointer or a nonzero reserved word; reservations without signals, with a fixed plan, with actuation or with advice; n_per outside
 * 1..64 or n_per n_junctions != P; n_mgr < 1, detect < 1 or patience < 0; conflict not symmetric, with a diagonal bit or with bits at or
 * above n_groups; lane without its own bit, not symmetric or with bits at or above n_groups (conflict, lane and mgr_time are read back
 * once per call; the per-agent, per-junction and per-point words are not -- a bad word is data, never a GPU fault); the signals' own
 * refusals of n_groups, n_points and brake; the agent-sharded layout; more than one linearisation pass. */
#define MPCX_RESERVE_PER_MAX 64
typedef struct {
    const int32_t *path_exit;    /* n_points: route-local index at which a vehicle on this point has left the crossing, -1 = none */
    const int32_t *conflict;     /* n_groups: bit h of word g = movements g and h may not hold the crossing together */
    const int32_t *lane;         /* n_groups: bit h of word g = movements g and h queue in the same approach lane */
    const int32_t *mgr_time;     /* n_mgr x 2: (detect in path points, patience in steps) */
    const int32_t *mgr_of;       /* n_junctions: the manager of junction j */
    int32_t *grant;              /* P, caller-owned, in-out, zero-initialised: 1 = the agent holds a reservation */
    int32_t *since;              /* P, caller-owned, in-out, initialised to -1: the clock value of the agent's first request */
    int32_t *clock;              /* n_junctions, caller-owned, in-out, zero-initialised */
    int32_t *occupied;           /* n_junctions, out: the mask of movements that hold the crossing */
    int32_t *queued;             /* n_junctions, out: the number of requesters denied this step */
    int32_t n_per, n_junctions, n_mgr, reserved;     /* reserved: 0 */
} mpcx_reservation;
/* the widest entry point: mpcx_closed_loop_run_intent with the reservation stage */
int32_t mpcx_closed_loop_run_reserved(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *cl,
                                      const mpcx_run_log *log /*or NULL*/, const mpcx_closed_loop_opts *opts /*or NULL*/,
                                      const mpcx_retire *retire /*or NULL*/, const mpcx_scene *scene /*or NULL*/,
                                      const mpcx_admit *admit /*or NULL*/, const mpcx_respawn *respawn /*or NULL*/,
                                      const mpcx_routes *routes /*or NULL*/, const mpcx_precedence *precedence /*or NULL*/,
                                      const mpcx_signals *signals /*or NULL*/, const mpcx_actuation *actuation /*or NULL*/,
                                      const mpcx_advice *advice /*or NULL*/, const mpcx_intent *intent /*or NULL*/,
                                      const mpcx_reservation *reservation /*or NULL*/, int32_t n_steps, int32_t use_graph);
/* one step's reservation stage alone (what mpcx_closed_loop_run_reserved enqueues between the conflict search and the window stage); the
 * arguments of mpcx_signal_step_batch plus the reservation.  Both structs are checked as above. */
int32_t mpcx_reserve_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const int32_t *path_off /*P*/,
                                const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *cut_len /*P*/,
                                const int32_t *done /*P or NULL*/, const mpcx_signals *signals, const mpcx_reservation *reservation);

/* ---- car following: an agent keeps a standstill distance and a time gap to the car ahead of it on its own path.  The conflict search
 * knows no leader -- it cuts the path where a prediction of the car in front meets the ego's own full-throttle prediction --, so a queue
 * behind a stop line, a platoon and two streams that merge into one arm have nothing that separates them.  With following on, one launch
 * (follow_kernel, csrc/mpcx_follow.hip; the rule is csrc/mpcx_follow_core.h) behind the signal / actuated / reserve stage -- behind the
 * conflict search where there are no signals -- finds every agent's leader and lowers its cut_len, and in MPCX_STOP_SPEED one more
 * (follow_clamp_kernel) behind every window stage caps row 2 of its xref.  The stage attaches to the CONTEXT (mpcx_set_following), as the
 * linearisation passes and the tuning rows do: every mpcx_closed_loop_run* entry point runs it while it is set.
 * For agent q with done[q] == 0 (otherwise only "no leader" is written): THE OTHERS are the rows of its pool window other than obs_skip[q],
 * in row order, the first MPCX_MAX_OBS of them, rows outside the pool or with absent[r] != 0 left out; agents and scripted actors alike,
 * obs6 as the head of this step packed it.  (1) k*(r) = the k in [traj_idx[q], min(traj_idx[q] + reach, path_len[q] - 1)] of q's full path
 * that minimises dx dx + dy dy to (x_r, y_r), the lowest k of equals.  (2) r is a candidate if k*(r) > traj_idx[q], the minimum is <=
 * lateral^2 and |wrap(yaw_path[k*] - yaw_r)| <= heading (wrap: 2 pi subtracted or added at most 33 times; no sin / cos).  (3) the leader is
 * the candidate with the smallest k*, the lowest pool row of equals: leader[q] = its row, gap[q] = (k* - traj_idx[q]) dl, v_l =
 * max(obs6[r][2], 0).  (4) with v = max(state[q][2], 0): s = k* - ceil((standstill + time_gap v) / dl) in MPCX_STOP_CUT, s = k* -
 * ceil(standstill / dl) in MPCX_STOP_SPEED; s is clamped to >= traj_idx[q] + 1 and cut_len[q] = min(cut_len[q], s).  (5) cap[q] =
 * max(v_min, -brake time_gap + sqrt(brake^2 time_gap^2 + v_l^2 + 2 brake max(gap - standstill, 0))), Gipps' safe speed.  No leader: leader
 * -1, gap -1.0, cap 0.0, cut_len untouched.  (6) MPCX_STOP_SPEED: every entry of row 2 of q's xref becomes fmin(entry, cap[q]) where
 * cap[q] > 0.  Precedence words are not consulted.  Host and device agree bit for bit.
 * NULL or an all-zero struct: off -- the loop enqueues exactly the launches of a context that never had it, with the same arguments.  The
 * cached graph's key covers the struct by value, and a run with the stage on does not take step fusion.  MPCX_E_INVALID ("following: ...")
 * from the run or the stage call before anything is launched, whatever n_steps is: leader, gap or cap NULL; n_rows != P; standstill, brake,
 * lateral or heading not finite or not positive; time_gap not finite or negative; v_min not finite or not positive; reach outside
 * 1..MPCX_MAX_REMAINING; a nonzero reserved word; the agent-sharded layout. */
typedef struct {
    int32_t *leader;             /* n_rows = P, caller-owned, out: the pool row of agent q's leader in the last step, -1 = none */
    double *gap;                 /* n_rows, out: the distance to it along q's path (m), -1.0 = none */
    double *cap;                 /* n_rows, out: the safe speed behind it (m/s), 0.0 = none */
    double standstill;           /* distance kept to a leader at rest (> 0, m) */
    double time_gap;             /* ... plus this many seconds of the follower's own speed (>= 0, s) */
    double brake;                /* the deceleration both cars are taken to brake with (> 0, m/s^2) */
    double v_min;                /* the cap is never below this (> 0, m/s) */
    double lateral;              /* a row counts if it is within this distance of the path (> 0, m) */
    double heading;              /* ... and heads along it within this angle (> 0, rad) */
    int32_t reach;               /* path points ahead that are scanned (1..MPCX_MAX_REMAINING) */
    int32_t n_rows, reserved;    /* reserved: 0 */
} mpcx_following;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_following(mpcx_ctx *ctx, const mpcx_following *following /*NULL or all-zero = off*/);

/* ---- the near-miss log: who came close to whom, how close, and how many frames from a predicted contact.  The run log keeps one clearance
 * per agent and step and says nothing of the other vehicle; a looming contact is invisible until the discs overlap.  With the safety stage
 * on, one launch (safety_kernel, csrc/mpcx_safety.hip; the rule is csrc/mpcx_safety_core.h) directly behind the conflict search -- before
 * the hold stage -- finds for every driving agent the vehicle nearest to it and the first predicted contact, keeps a per-agent table of
 * ENCOUNTERS in device memory, and mpcx_safety_summary reduces the tables to a CONFLICT MATRIX per pair of movements.  The stage changes no
 * decision of the loop and no existing buffer: it reads obs6, the prediction of every pool row as the conflict search read it (after the
 * intent stage), traj_idx as the conflict search left it, path_off, state, done and absent, and writes only its own words, every one a word
 * of agent q.  It attaches to the CONTEXT (mpcx_set_safety), as following does: every mpcx_closed_loop_run* entry point runs it while set.
 * For agent q with own row o = obs_skip[q]: THE OTHERS are following's -- the rows of its pool window other than o, in row order, the first
 * MPCX_MAX_OBS of them, rows outside the pool or with absent[r] != 0 left out; precedence words are not consulted.  NOT MEASURED: done[q]
 * != 0, o outside the pool, absent[o] != 0, no others -- every per-step word is "none", the open encounter is closed, tick[q] advances.
 * (1) c_now = the minimum over the others and the 2 x 2 pairs of discs of hypot(..) - 2 radius at the poses of obs6 -- the run log's
 * clearance of the step, bit for bit --, r_now its row, the lowest slot of equals; nobody: +inf, -1.  (2) d2(r, k) = the minimum over the
 * 2 x 2 pairs of discs of dx dx + dy dy between frames k of rows o and r of the prediction; k(r) = the lowest k in [0, pred_steps) with
 * d2(r, k) < (2 radius)^2; (k_ttc, r_ttc) = the smallest k(r), the lowest slot of equals; none: -1, -1.  Frame k is the pose (k + 1) dt
 * ahead.  (3) partner[q] = r_now, clearance[q] = c_now, ttc_row[q] = r_ttc, ttc_frame[q] = k_ttc.  (4) critical = c_now < near or 0 <=
 * k_ttc < ttc_frames, the encounter's partner p = r_now if c_now < near, else r_ttc; enc_row[q] is the partner of the open encounter.  Not
 * critical: enc_row[q] = -1.  Critical and enc_row[q] != p: event e = n_events[q]++ opens, enc_row[q] = p, and if e < capacity its record is
 * written (an event beyond capacity is counted and tracked, not stored): ev_i32[q][e] = tick[q] (open), tick[q] (last), p, row_agent[p]
 * (-1 for a scripted actor), path_off[q], path_off[row_agent[p]] (or -1), traj_idx[q], k_ttc; ev_f64[q][e] = c_now, state[q].v.  Critical
 * and enc_row[q] == p with a stored record: word 1 = tick[q], word 7 = the smaller non-negative of itself and k_ttc, ev_f64[0] =
 * fmin(itself, c_now).  Last, always: tick[q]++.  Host and device agree bit for bit on the integer words.
 * NULL or an all-zero struct: off -- the loop enqueues exactly the launches of a context that never had it, with the same arguments.  The
 * cached graph's key covers the struct by value, and a run with the stage on does not take step fusion.  MPCX_E_INVALID ("safety: ...")
 * from the run or the stage call before anything is launched, whatever n_steps is: a required pointer NULL (the event arrays only with
 * capacity > 0); n_rows != P; n_pool not the run's pool rows; near not finite or negative; ttc_frames outside 0..pred_steps; capacity < 0;
 * a radius that is not finite; a nonzero reserved word; no obs_skip; the agent-sharded layout. */
typedef struct {
    int32_t *partner;            /* n_rows = P, caller-owned, out: the pool row nearest to agent q in the last step, -1 = none */
    double *clearance;           /* n_rows, out: its clearance (m), +inf = none */
    int32_t *ttc_row;            /* n_rows, out: the pool row of the first predicted contact, -1 = none */
    int32_t *ttc_frame;          /* n_rows, out: its frame; the contact is (frame + 1) dt ahead; -1 = none */
    int32_t *tick;               /* n_rows, in-out (zero-initialised): steps the stage has run for the agent */
    int32_t *enc_row;            /* n_rows, in-out (initialised to -1): the partner row of the open encounter */
    int32_t *n_events;           /* n_rows, in-out (zero-initialised): encounters opened so far, stored or not */
    int32_t *ev_i32;             /* n_rows x capacity x 8, out: the event records' integer words */
    double *ev_f64;              /* n_rows x capacity x 2, out: minimum clearance of the event, the agent's speed when it opened */
    const int32_t *row_agent;    /* n_pool: the agent that owns pool row r, -1 (or anything outside [0, P)) for a scripted actor */
    double near;                 /* an encounter is open while the clearance is below this (finite, >= 0, m) */
    int32_t ttc_frames;          /* ... or a contact is predicted in fewer frames than this (0..pred_steps) */
    int32_t capacity;            /* event records per agent (>= 0; 0: ev_i32 and ev_f64 may be NULL) */
    int32_t n_rows, n_pool, reserved;    /* reserved: 0 */
} mpcx_safety;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_safety(mpcx_ctx *ctx, const mpcx_safety *safety /*NULL or all-zero = off*/);
/* one step's safety stage alone (what the closed loop enqueues behind the conflict search).  pred: n_obs_pool x ip->pred_steps x 4 doubles
 * ([row][frame][2 discs][2]), DEVICE, or NULL = the context's own prediction as its last conflict search left it; ip gives radius,
 * circle_centers, pred_steps and dt.  The struct is the argument's, not the context's, and is checked as above. */
int32_t mpcx_safety_step_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state /*P,4*/,
                               const int32_t *path_off /*P*/, const int32_t *traj_idx /*P*/, const int32_t *done /*P or NULL*/,
                               int32_t n_obs_pool, const double *obs6 /*NOBS,6*/, const double *pred /*NOBS,pred_steps,4 or NULL*/,
                               const int32_t *obs_off /*P*/, const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P*/,
                               const int32_t *absent /*NOBS or NULL*/, const mpcx_safety *safety);
/* the conflict matrix, reduced on the device (one wavefront per instance of A consecutive agents): over the stored events (e <
 * min(n_events[q], capacity)) per pair (class of q, class of the partner).  The class of an event side is the route r with route_off[r] ==
 * its path_off word (words 4 and 5), the lowest r of equals; class R = no route (an actor, or an unknown offset).  out_i64[b][R+1][R+1][3]:
 * events, events with minimum clearance < 0, events whose word 7 >= 0.  out_f64[b][R+1][R+1][2]: the minimum of the minimum clearance (a NaN
 * is skipped; +inf: no events), the minimum over the events with word 7 >= 0 of (word 7 + 1) dt (+inf: none).  Integer sums and minima
 * only: exact whatever the lane mapping.  Every pointer is a DEVICE pointer. */
int32_t mpcx_safety_summary(mpcx_ctx *ctx, int32_t P, int32_t A, int32_t capacity, int32_t R, const int32_t *route_off /*R*/, double dt,
                            const int32_t *n_events /*P*/, const int32_t *ev_i32 /*P,capacity,8*/, const double *ev_f64 /*P,capacity,2*/,
                            int64_t *out_i64 /*P/A,R+1,R+1,3*/, double *out_f64 /*P/A,R+1,R+1,2*/);

/* ---- line of sight: buildings hide cars from each other.  Without it the conflict search of agent q reads the prediction of every present
 * row of its window, wherever that car is.  With the sight stage on, one launch (sight_kernel, csrc/mpcx_sight.hip; the rule is
 * csrc/mpcx_sight_core.h) behind the pack of the pool and the intent stage and in front of the conflict search decides, per agent, which rows
 * of its window it sees, and the conflict search takes its SIGHT instantiation (csrc/mpcx_interaction_sight.hip), which ANDs the agent's word
 * onto its ballot of present rows: a row agent q cannot see is, for q and only for q, an absent row.  It attaches to the CONTEXT
 * (mpcx_set_sight), as following and the near-miss log do: every mpcx_closed_loop_run* entry point runs it while set, and it needs
 * retirement and a scene (the conflict search's list of present rows is the scene's).  The per-stage entry points mpcx_interaction_batch and
 * mpcx_interaction_batch_intent carry no scene and therefore never take the SIGHT instantiation.
 * For agent q with own row o = obs_skip[q], eye E = (state[q].x, state[q].y) and window offset j < min(obs_cnt[q], 64), r = obs_off[q] + j:
 * NOT A CANDIDATE if r is outside the pool, r == o or absent[r] != 0 -- bit j = 0, not counted.  OUT OF RANGE if dx dx + dy dy > range range
 * with (dx, dy) = T - E, T = the (x, y) of obs6[r]: hidden (no trig, no car extent: the reference point stands for the car).  In range and
 * heard[r] != 0: seen, the occluders are not consulted (a connected vehicle announces its pose).  Otherwise seen iff no occluder of the
 * agent's set blocks the segment E -> T.  OCCLUDERS are convex polygons as half-plane rows (a, b, c), inside <=> a x + b y + c <= 0, CSR:
 * occluder i has the rows hp[3 hp_off[i] .. 3 hp_off[i + 1]) and the host-computed box box[4 i ..] = (x0, y0, x1, y1); set s is the occluders
 * set_off[s] .. set_off[s + 1), agent q's set is set_of[q]; an empty set is an open junction, so a sweep of worlds is one batch.  An occluder
 * is skipped if the segment's own box misses its box (four comparisons, part of the rule); else Cyrus-Beck: t_in = 0, t_out = 1, per row den =
 * a dx + b dy, num = -((a Ex + b Ey) + c); den == 0 and num < 0: outside, the polygon is finished; den > 0: t_out = min(t_out, num / den); den
 * < 0: t_in = max(t_in, num / den); it blocks iff it was not left early and t_in < t_out (strict: a grazing segment is not blocked; an eye
 * or a target inside is blocked; T == E is blocked iff E is inside).  A shrink of the occluders (a car whose centre is just behind a corner
 * is seen by its body) is applied by the host when it builds the table.  OUTPUTS, every one a word of agent q, no atomics: sight[q] bit j =
 * the row at window offset j is seen, n_seen[q] its population count, n_hidden[q] the candidates that are not seen; a retired agent
 * (done[q] != 0) writes 0, 0, 0.  Host and device agree bit for bit.
 * NULL or an all-zero struct: off -- the loop enqueues exactly the launches of a context that never had it, with the same arguments.  The
 * cached graph's key covers the struct by value, and a run with the stage on does not take step fusion.  MPCX_E_INVALID ("sight: ...") from
 * the run or the stage call before anything is launched, whatever n_steps is: a required pointer NULL (heard may be NULL; hp and box only
 * with n_occ > 0); n_rows != P; n_pool not the run's pool rows; range NaN or not positive (+inf is allowed); n_sets < 1; n_occ < 0; set_off
 * not non-decreasing from 0 within 0..n_occ; hp_off not non-decreasing from 0; a run without retirement and a scene; a nonzero reserved
 * word; no obs_skip (from the stage call; in a run the scene it lives on refuses that first, as it refuses the agent-sharded layout).  The
 * two offset tables are read back from the device for their check (two blocking copies) ONCE per struct: the context remembers the
 * pointers and counts that passed and forgets them when mpcx_set_sight is given a struct that differs from the one it holds, so run(1) in
 * a loop reads nothing back.  Do not change the tables in place while set; after mpcx_set_sight(NULL) a new mpcx_set_sight has them
 * checked again.  set_of is NOT read back: the Python layer checks it on the host, and the rule takes a word outside [0, n_sets) as the
 * empty set, so a bad word never reads outside the tables. */
typedef struct {
    uint64_t *sight;             /* n_rows = P, caller-owned, out: bit j = the row at window offset j of agent q is seen */
    int32_t *n_seen, *n_hidden;  /* n_rows each, out: rows seen; candidates not seen */
    const double *hp;            /* hp_off[n_occ] x 3: the half-plane rows (a, b, c) of every occluder */
    const int32_t *hp_off;       /* n_occ + 1: occluder i has the rows hp_off[i] .. hp_off[i + 1] */
    const double *box;           /* n_occ x 4: (x0, y0, x1, y1) of every occluder */
    const int32_t *set_off;      /* n_sets + 1: set s is the occluders set_off[s] .. set_off[s + 1] */
    const int32_t *set_of;       /* n_rows: the set of agent q */
    const int32_t *heard;        /* n_pool or NULL: != 0 = the row is seen wherever it is in range */
    double range;                /* the sensor range (m); > 0, +inf allowed */
    int32_t n_occ, n_sets, n_rows, n_pool, reserved;    /* reserved: 0 */
} mpcx_sight;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_sight(mpcx_ctx *ctx, const mpcx_sight *sight /*NULL or all-zero = off*/);
/* one step's sight stage alone (what the closed loop enqueues in front of the conflict search), on the pool as packed in obs6.  The struct
 * is the argument's, not the context's, and is checked as above. */
int32_t mpcx_sight_step_batch(mpcx_ctx *ctx, int32_t P, const double *state /*P,4*/, const int32_t *done /*P or NULL*/, int32_t n_obs_pool,
                              const double *obs6 /*NOBS,6*/, const int32_t *obs_off /*P*/, const int32_t *obs_cnt /*P*/,
                              const int32_t *obs_skip /*P*/, const int32_t *absent /*NOBS or NULL*/, const mpcx_sight *sight);

/* ---- keep clear: a car whose light lets it go waits at its line while the crossing is occupied by a movement that conflicts with its own.
 * The signal hold looks at the light and nothing else, and the conflict search sees a late car of the phase before only as a prediction and
 * only once the released car is moving: under a two-phase plan the first car of a phase drives into a car that is still crossing.  With the
 * keep-clear stage on, one launch (keepclear_kernel, csrc/mpcx_keepclear.hip; the rule is csrc/mpcx_keepclear_core.h) directly behind the
 * hold (signal_kernel or actuated_signal_kernel) and in front of the following stage works out, per junction, which movements are inside
 * the crossing and holds such a car at its stop line by the cut the signal hold makes.  It costs nothing when the box is empty, where a
 * longer all-red costs capacity in every cycle.  It attaches to the CONTEXT (mpcx_set_keepclear), as following, the near-miss log and line
 * of sight do: every mpcx_closed_loop_run* entry point runs it while set; it needs signals (fixed plan or actuated) and is refused beside
 * a reservation, whose manager already keeps the crossing clear.
 * The signal groups stay what they are.  A junction is n_per consecutive agents, n_per <= 64: junction j owns agents [j n_per, (j + 1)
 * n_per), n_per n_junctions = P.  Tables: path_move[n_points] the movement of the route on that path point, at most
 * MPCX_SIGNAL_GROUPS_MAX movements; path_exit[n_points] the route-local index e at which a vehicle on this point has left the crossing, -1
 * if no crossing lies ahead or under the point; conflict[n_moves], bit h of word g set when movements g and h may not be in the crossing
 * together (symmetric, no diagonal).  The stop line (path_stop), held and brake are the run's mpcx_signals'.  State, caller-owned device
 * memory: waited[P] in-out, zero-initialised; boxed[P] out (0 / 1); occupied[n_junctions] out (the movements inside the crossing);
 * n_boxed[n_junctions] out.
 * Per junction and step: (1) every agent q, with ti = traj_idx[q] as this step's conflict search left it, i = path_off[q] + ti, s =
 * path_stop[i], m = path_move[i], e = path_exit[i]: OUT if done[q] != 0 (retired, or waiting for admission), i outside [0, n_points), e <
 * 0, e > path_len[q], ti >= e, m outside [0, n_moves), or ti < s with s >= path_len[q]; INSIDE if not OUT and (s < 0 or ti >= s); otherwise
 * APPROACH.  (2) occ = OR of 1 << m over the INSIDE agents.  (3) an APPROACH agent is a candidate if held[q] == 0 as this step's hold left
 * it, s - ti <= detect and (conflict[m] & occ) != 0; a candidate is BOXED if waited[q] != 0 -- a car that stood at its line in the step
 * before does not start into an occupied box, the amber rule's stickiness -- or if it can stop, (double)(s - ti) dl >= v v / (2.0 brake)
 * with v = state[q][2], the signal hold's own expression; otherwise it is free: a car that arrives at speed on green and cannot stop any
 * more is left to the conflict search, as on amber.  Boxed: boxed[q] = 1, cut_len[q] = min(cut_len[q], s); everybody else: boxed[q] = 0,
 * cut_len untouched.  (4) waited[q] = 1 for an APPROACH agent with held[q] != 0 or boxed[q] != 0, 0 for everybody else.  (5) occupied[j] =
 * occ, n_boxed[j] = the number boxed.  The comparison of (3) is the only floating point.  Host and device agree bit for bit.
 * The stage writes no word of another stage: held stays the signal stage's, so the actuated controller's calls and the advice stage read
 * what they read without it.  NULL or an all-zero struct: off -- the loop enqueues exactly the launches of a context that never had it,
 * with the same arguments.  The cached graph's key covers the struct by value (it has no padding: six int32 close its 80 bytes), and a run
 * with the stage on does not take step fusion.  MPCX_E_INVALID ("keepclear: ...") from the run or the stage call before anything is
 * launched, whatever n_steps is: no signals; a reservation in the run; one of the seven pointers (or the signals' path_stop or held) NULL;
 * n_per outside 1..64 or n_per n_junctions != P; n_moves outside 1..MPCX_SIGNAL_GROUPS_MAX; n_points not the signals'; detect < 1; a
 * conflict word with bits at or above n_moves, with its own bit, or not symmetric; more than one linearisation pass; the agent-sharded
 * layout; a nonzero reserved word.  The conflict table is read back from the device for its check (one blocking copy) ONCE per struct: the
 * context remembers the pointer and count that passed and forgets them when mpcx_set_keepclear is given a struct that differs from the
 * one it holds, so run(1) in a loop reads nothing back.  Do not change the table in place while set; after mpcx_set_keepclear(NULL) a new
 * mpcx_set_keepclear has it checked again.  The per-agent, per-junction and per-point words are not read back -- a bad word is data (OUT),
 * never a GPU fault. */
#define MPCX_KEEPCLEAR_PER_MAX 64
typedef struct {
    const int32_t *path_move;    /* n_points: the movement of the route on this path point */
    const int32_t *path_exit;    /* n_points: route-local index at which a vehicle on this point has left the crossing, -1 = none */
    const int32_t *conflict;     /* n_moves: bit h of word g = movements g and h may not be in the crossing together */
    int32_t *boxed;              /* P, caller-owned, out: 1 = the agent was held at its line by this stage in the last step */
    int32_t *waited;             /* P, caller-owned, in-out, zero-initialised: 1 = the agent stood at its line (held or boxed) in the last step */
    int32_t *occupied;           /* n_junctions, out: the mask of movements inside the crossing */
    int32_t *n_boxed;            /* n_junctions, out: the number of agents boxed this step */
    int32_t detect;              /* an agent is looked at from this many path points before its line on (>= 1) */
    int32_t n_per, n_junctions, n_moves, n_points, reserved;     /* reserved: 0 */
} mpcx_keepclear;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_keepclear(mpcx_ctx *ctx, const mpcx_keepclear *keepclear /*NULL or all-zero = off*/);
/* one step's keep-clear stage alone (what the closed loop enqueues behind the hold); the arguments of mpcx_signal_step_batch plus the
 * struct, called behind mpcx_signal_step_batch or mpcx_actuated_step_batch on the same signals: it reads their held as that call left it.
 * The struct is the argument's, not the context's, and is checked as above (its conflict table in every call). */
int32_t mpcx_keepclear_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const int32_t *path_off /*P*/,
                                  const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *cut_len /*P*/,
                                  const int32_t *done /*P or NULL*/, const mpcx_signals *signals, const mpcx_keepclear *keepclear);

/* ---- priority road: a car of a minor movement waits at its stop line until the conflicting movements of smaller rank leave it a gap.
 * give_way('entry') ranks by order of entry and give_way(order=) by slot, and the conflict search cuts a path only where two predictions
 * meet: a minor-road car pulls out in front of a major-road car, which then yields to it.  With the priority stage on, one launch
 * (priority_kernel, csrc/mpcx_priority.hip; the rule is csrc/mpcx_priority_core.h) in the hold's place -- behind the conflict search and
 * the safety stage, in front of the following stage -- holds such a car at its line by the cut the signal hold makes, in both stop modes.
 * It attaches to the CONTEXT (mpcx_set_priority), as following, the near-miss log, line of sight and keep clear do: every
 * mpcx_closed_loop_run* entry point runs it while set.  A junction is run by lights, by a manager, or by priority: the stage is refused
 * beside signals, actuation or a reservation, so the stop lines are its own table.
 * A junction is n_per consecutive agents, n_per <= 64: junction j owns agents [j n_per, (j + 1) n_per), n_per n_junctions = P.  Tables:
 * path_stop[n_points], path_move[n_points], path_exit[n_points] as mpcx_signals' and mpcx_keepclear's (the route-local index of the next
 * stop line at or after the point, -1 = none; the movement of the route, at most MPCX_SIGNAL_GROUPS_MAX movements; the route-local index at
 * which a vehicle on the point has left the crossing, -1 = none); conflict[n_moves], bit h of word g set when movements g and h cross
 * (symmetric, no diagonal); rank[n_moves] >= 0, a smaller rank goes first; gap[n_moves], finite and >= 0, the critical gap in seconds of
 * movement m when it gives way.  Scalars: v_floor (> 0, the least speed an approaching car is taken to have), brake (> 0), detect (>= 1
 * path point).  State, caller-owned device memory: waited[P] in-out, zero-initialised; yielding[P] out (0 / 1); blocker[P] out, an agent
 * index, -1 = none; lag[P] out, seconds, +inf = none; occupied[n_junctions] out (the movements inside the crossing); n_yielding[n_junctions]
 * out.
 * Per junction and step, everything is read before anything is written: (1) every agent q is OUT, INSIDE or APPROACH with (m, s, ti)
 * exactly as the keep-clear stage classifies it (above), done[q] != 0 being OUT.  (2) an agent r that is not OUT has eta_r = 0.0 if INSIDE,
 * else (double)(s_r - ti_r) dl / fmax(state[r][2], v_floor); occ = OR of 1 << m over the INSIDE agents.  (3) an APPROACH agent q with
 * s_q - ti_q <= detect: lag[q] = the minimum of eta_r over the agents r != q of the junction that are not OUT, have rank[m_r] < rank[m_q]
 * and bit m_r of conflict[m_q] set; blocker[q] = the agent that attains it, the lowest index among equals; none: +inf and -1.  q is
 * THREATENED iff lag[q] < gap[m_q].  Everybody else: lag = +inf, blocker = -1, yielding = 0, waited = 0.  (4) a threatened q YIELDS if
 * waited[q] != 0 or if it can still stop, (double)(s - ti) dl >= v v / (2.0 brake), the signal hold's own expression; otherwise it is free
 * and left to the conflict search, as on amber.  Yields: yielding[q] = 1, cut_len[q] = min(cut_len[q], s).  (5) waited[q] = yielding[q].
 * (6) occupied[j] = occ, n_yielding[j] = the number yielding.  eta is one multiply and one IEEE division, the rest comparisons: host and
 * device agree bit for bit, lag included.  Equal ranks stay with the conflict search.
 * The stage writes no word of another stage and only lowers cut_len.  NULL or an all-zero struct: off -- the loop enqueues exactly the
 * launches of a context that never had it, with the same arguments.  The cached graph's key covers the struct by value (it has no padding:
 * twelve pointers, two doubles and six int32 are its 136 bytes), and a run with the stage on does not take step fusion.  MPCX_E_INVALID
 * ("priority: ...") from the run or the stage call before anything is launched, whatever n_steps is: one of the twelve pointers NULL;
 * n_per outside 1..64 or n_per n_junctions != P; n_moves outside 1..MPCX_SIGNAL_GROUPS_MAX; n_points < 1; detect < 1; v_floor or brake not
 * finite or not positive; a nonzero reserved word; signals, actuation or a reservation in the run; the agent-sharded layout; more than one
 * linearisation pass; a conflict word with bits at or above n_moves, with its own bit, or not symmetric; a negative rank; a gap that is
 * not finite or is negative.  The three per-movement tables are read back from the device for their check (blocking copies) ONCE per
 * struct: the context remembers the pointers and count that passed and forgets them when mpcx_set_priority is given a struct that differs
 * from the one it holds, so run(1) in a loop reads nothing back.  Do not change the tables in place while set.  The per-agent,
 * per-junction and per-point words are not read back -- a bad word is data (OUT), never a GPU fault. */
#define MPCX_PRIORITY_PER_MAX 64
typedef struct {
    const int32_t *path_stop;    /* n_points: route-local index of the next stop line at or after this path point, -1 = none */
    const int32_t *path_move;    /* n_points: the movement of the route on this path point */
    const int32_t *path_exit;    /* n_points: route-local index at which a vehicle on this point has left the crossing, -1 = none */
    const int32_t *conflict;     /* n_moves: bit h of word g = movements g and h cross */
    const int32_t *rank;         /* n_moves: >= 0, a smaller rank goes first */
    const double *gap;           /* n_moves: the critical gap in seconds of the movement when it gives way (finite, >= 0) */
    int32_t *waited;             /* P, caller-owned, in-out, zero-initialised: 1 = the agent yielded in the last step */
    int32_t *yielding;           /* P, caller-owned, out: 1 = the agent was held at its line by this stage in the last step */
    int32_t *blocker;            /* P, out: the agent whose arrival is the lag, -1 = none */
    double *lag;                 /* P, out: seconds until the first conflicting agent of smaller rank is at its line, +inf = none */
    int32_t *occupied;           /* n_junctions, out: the mask of movements inside the crossing */
    int32_t *n_yielding;         /* n_junctions, out: the number of agents yielding this step */
    double v_floor;              /* m/s, > 0: an approaching agent is taken to drive at least this fast */
    double brake;                /* m/s^2, > 0: the deceleration of the can-stop test */
    int32_t detect;              /* an agent is looked at from this many path points before its line on (>= 1) */
    int32_t n_per, n_junctions, n_moves, n_points, reserved;     /* reserved: 0 */
} mpcx_priority;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_priority(mpcx_ctx *ctx, const mpcx_priority *priority /*NULL or all-zero = off*/);
/* one step's priority stage alone (what the closed loop enqueues in the hold's place).  The struct is the argument's, not the context's,
 * and is checked as above (its per-movement tables in every call). */
int32_t mpcx_priority_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const int32_t *path_off /*P*/,
                                 const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *cut_len /*P*/,
                                 const int32_t *done /*P or NULL*/, const mpcx_priority *priority);

/* ---- stop signs: a car of a signed movement comes to a standstill at its stop line, and the cars that have stopped leave in the order in
 * which they stopped; in the two-way case a stopped car also waits for a gap in the unsigned road.  The priority road holds a minor-road
 * car only while a conflicting car is within its gap -- on an empty road it drives through its line, under a saturated major stream it
 * starves --, and a reservation orders cars by their first request without making them stop.  With the stop-sign stage on, one launch
 * (stopsign_kernel, csrc/mpcx_stopsign.hip; the rule is csrc/mpcx_stopsign_core.h) in the hold's place -- behind the conflict search and
 * the safety stage, in front of the following stage, where priority_kernel runs -- holds a signed car at its line by the cut the signal
 * hold makes until it has stood there and its turn has come, in both stop modes.  It attaches to the CONTEXT (mpcx_set_stopsign), as the
 * priority road does: every mpcx_closed_loop_run* entry point runs it while set.  A junction is run by lights, by a manager, by priority,
 * or by signs: the stage is refused beside signals, actuation, a reservation or the priority road, so the stop lines are its own table.
 * A junction is n_per consecutive agents, n_per <= 64: junction j owns agents [j n_per, (j + 1) n_per), n_per n_junctions = P.  Tables:
 * path_stop[n_points], path_move[n_points], path_exit[n_points] as mpcx_priority's; conflict[n_moves], bit h of word g set when movements
 * g and h cross (symmetric, no diagonal); lane[n_moves], bit h of word g set when they queue in the same approach lane (bit g of word g
 * is set), as mpcx_reservation's; sign[n_moves], 0 = uncontrolled, 1 = stop sign; gap[n_moves], finite and >= 0, the critical gap in
 * seconds of a signed movement against unsigned traffic.  Scalars: v_stop (> 0: a car at or below this speed stands), zone (>= 1: path
 * points before the line within which a standstill counts as the stop), detect (>= zone), brake (> 0), v_floor (> 0), patience (>= 0,
 * steps).  State, caller-owned device memory, in-out: stopped_at[P], the junction clock at which the agent completed its stop, -1 = not
 * yet, -1-initialised; go[P] (0 / 1), stopping[P] (0 / 1: the hold word and last step's stickiness), clock[n_junctions],
 * ran[n_junctions] (a running count of the cars that entered a signed movement without a release), all zero-initialised.  Out: lag[P]
 * (seconds, +inf = none), blocker[P] (an agent index, -1 = none), occupied[n_junctions], n_waiting[n_junctions].
 * Per junction and step, everything is read before anything is written: (1) t = clock[j], a negative word counting as 0; clock[j] = t + 1,
 * wrapping as the reservation's clock does.  (2) every agent q is OUT, INSIDE or APPROACH with (m, s, ti) exactly as the keep-clear stage
 * classifies it on the stage's tables, done[q] != 0 being OUT; d = s - ti.  OUT: go = 0, stopped_at = -1, stopping = 0.  INSIDE: it
 * occupies m; with sign[m] != 0 and go == 0 it ran the sign and ran[j] counts it, once; then go = 1, stopped_at is left alone, stopping =
 * 0.  APPROACH on an unsigned movement: never held, go = 0, stopped_at = -1, stopping = 0; eta = (double)d dl / fmax(v, v_floor) is what
 * signed cars see of it.  APPROACH, signed, go != 0: it occupies m -- a release is never revoked --, stopping = 0.  APPROACH, signed, go ==
 * 0, d > detect: stopped_at = -1, stopping = 0.  APPROACH, signed, go == 0, d <= detect: SUBJECT; if stopped_at < 0, d <= zone and v <=
 * v_stop then stopped_at = t; a subject agent with stopped_at >= 0 REQUESTS.  (3) occ = OR of 1 << m over the occupying agents.  (4) a
 * requester q: lag[q] = the lexicographic minimum of (eta_r, r) over the unsigned APPROACH agents r of the junction with bit m_r of
 * conflict[m_q] set, blocker[q] the agent that attains it, none: +inf and -1; everybody else: +inf and -1.  (5) the requesters in ascending
 * order of (stopped_at, index within the junction), from ahead = blocked = 0: released (go = 1, occ |= 1 << m) if (conflict[m] & (occ |
 * blocked)) == 0, (lane[m] & ahead) == 0 and lag >= gap[m]; otherwise denied, ahead |= 1 << m, and if aged, (int64)t - stopped_at >=
 * patience, also blocked |= 1 << m.  (6) a subject agent with go == 0 after (5) is held if stopping[q] != 0 from the step before or if it
 * can still stop, (double)d dl >= v v / (2.0 brake), the signal hold's own expression: stopping = 1, cut_len[q] = min(cut_len[q], s);
 * otherwise stopping = 0, the car is left to the conflict search and ran will count it.  (7) occupied[j] = occ, n_waiting[j] = the number
 * of agents with stopping != 0.  eta is one multiply and one IEEE division, the rest comparisons: host and device agree bit for bit, lag
 * included.
 * The stage writes no word of another stage and only lowers cut_len.  A slot reset by the respawn stages is OUT while it waits at the
 * gate, so the four agent words heal themselves.  NULL or an all-zero struct: off -- the loop enqueues exactly the launches of a context
 * that never had it, with the same arguments.  The cached graph's key covers the struct by value (it has no padding: sixteen pointers,
 * three doubles and eight int32 are its 184 bytes), and a run with the stage on does not take step fusion.  With the firm hold on, the
 * stop lines are this stage's and stopping is the hold word the mark launch reads.  MPCX_E_INVALID ("stopsign: ...") from the run or the
 * stage call before anything is launched, whatever n_steps is: one of the sixteen pointers NULL; a nonzero reserved word; n_per outside
 * 1..64 or n_per n_junctions != P; n_moves outside 1..MPCX_SIGNAL_GROUPS_MAX; n_points < 1; zone < 1 or zone > detect; patience < 0;
 * v_stop, brake or v_floor not finite or not positive; signals, actuation, a reservation or the priority road in the run; the
 * agent-sharded layout; more than one linearisation pass; a conflict or lane word with bits at or above n_moves; a conflict word with its
 * own bit or not symmetric; a lane word without its own bit; a sign that is neither 0 nor 1; a gap that is not finite or is negative.
 * The four per-movement tables are read back from the device for their check (blocking copies) ONCE per struct: the context remembers the
 * pointers and count that passed and forgets them when mpcx_set_stopsign is given a struct that differs from the one it holds, so run(1)
 * in a loop reads nothing back.  Do not change the tables in place while set.  The per-agent, per-junction and per-point words are not
 * read back -- a bad word is data (OUT), never a GPU fault. */
#define MPCX_STOPSIGN_PER_MAX 64
typedef struct {
    const int32_t *path_stop;    /* n_points: route-local index of the next stop line at or after this path point, -1 = none */
    const int32_t *path_move;    /* n_points: the movement of the route on this path point */
    const int32_t *path_exit;    /* n_points: route-local index at which a vehicle on this point has left the crossing, -1 = none */
    const int32_t *conflict;     /* n_moves: bit h of word g = movements g and h cross */
    const int32_t *lane;         /* n_moves: bit h of word g = movements g and h queue in the same approach lane (bit g of word g set) */
    const int32_t *sign;         /* n_moves: 0 = uncontrolled, 1 = stop sign */
    const double *gap;           /* n_moves: the critical gap in seconds of a signed movement against unsigned traffic (finite, >= 0) */
    int32_t *stopped_at;         /* P, caller-owned, in-out, -1-initialised: the junction clock at which the agent completed its stop */
    int32_t *go;                 /* P, caller-owned, in-out, zero-initialised: 1 = released (or inside) */
    int32_t *stopping;           /* P, caller-owned, in-out, zero-initialised: 1 = the agent was held at its line by this stage in the last step */
    int32_t *clock;              /* n_junctions, caller-owned, in-out, zero-initialised: the junction's step count */
    int32_t *ran;                /* n_junctions, caller-owned, in-out, zero-initialised: cars that entered a signed movement unreleased */
    double *lag;                 /* P, out: seconds until the first conflicting unsigned car is at its line, +inf = none */
    int32_t *blocker;            /* P, out: the agent whose arrival is the lag, -1 = none */
    int32_t *occupied;           /* n_junctions, out: the mask of movements inside the crossing or released into it */
    int32_t *n_waiting;          /* n_junctions, out: the number of agents held this step */
    double v_stop;               /* m/s, > 0: a car at or below this speed stands */
    double brake;                /* m/s^2, > 0: the deceleration of the can-stop test */
    double v_floor;              /* m/s, > 0: an approaching unsigned car is taken to drive at least this fast */
    int32_t zone;                /* path points before the line within which a standstill counts as the stop (>= 1) */
    int32_t detect;              /* an agent is looked at from this many path points before its line on (>= zone) */
    int32_t patience;            /* steps after which a denied requester blocks the movements that cross its own (>= 0) */
    int32_t n_per, n_junctions, n_moves, n_points, reserved;     /* reserved: 0 */
} mpcx_stopsign;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_stopsign(mpcx_ctx *ctx, const mpcx_stopsign *stopsign /*NULL or all-zero = off*/);
/* one step's stop-sign stage alone (what the closed loop enqueues in the hold's place): steps 1 - 7 above.  The struct is the argument's,
 * not the context's, and is checked as above (its per-movement tables in every call). */
int32_t mpcx_stopsign_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const int32_t *path_off /*P*/,
                                 const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *cut_len /*P*/,
                                 const int32_t *done /*P or NULL*/, const mpcx_stopsign *stopsign);

/* ---- firm hold: in MPCX_STOP_SPEED a car that a hold keeps at its stop line stops in front of it.  Every rule that stops a car at a line
 * (signals, actuation, a reservation, keep clear, the priority road, stop signs) lowers cut_len to the line's index s.  In MPCX_STOP_CUT the path ends
 * there; in MPCX_STOP_SPEED only the speed reference is zeroed from s on, and that does not hold a car: the window's position reference
 * advances by max(v, 10 / 3.6) dt whatever the car does and runs over the line, and the nearest-index search answers start + 1 for a car
 * that stands on start, so traj_idx climbs to s and the hold's "on or past the line" frees a car that stands 2 m before its line.  With the
 * stage on, two small launches (brake_mark_kernel behind the last hold stage and the following stage, in front of the window stage;
 * brake_clamp_kernel behind every window stage, beside the advice and following clamps; csrc/mpcx_brake.hip, the rule is
 * csrc/mpcx_brake_core.h) end a line-held agent's position reference on a stop point in front of its line, put a braking profile on its
 * speed reference and pin its index while it is physically behind the line.  It attaches to the CONTEXT (mpcx_set_braking), as
 * following, keep clear and the priority road do: every mpcx_closed_loop_run* entry point runs it while set.
 * Agent q is LINE-HELD in a step if done[q] == 0, one of the hold words that are on in THAT run is nonzero for it -- mpcx_signals.held
 * (signals, actuation, a reservation), mpcx_keepclear.boxed, mpcx_priority.yielding or, under stop signs, mpcx_stopsign.stopping in its
 * place (the two never run together); which of them are read follows the stages of the run
 * that is enqueued, not those at the time of mpcx_set_braking --, and s = path_stop[path_off[q] + traj_idx[q]] is a valid line ahead by
 * the hold's own test: path_off[q] + traj_idx[q] in [0, n_points), 0 <= traj_idx[q] < s < path_len[q] (path_stop and n_points: the
 * signals', else the priority road's, else the stop signs').  Then m = ceil(setback / dl), e = max(s - m, 2), E = path point e - 1.
 *   (a) the window stage builds q's window on full[:e], searching from min(target_ind[q], e - 1): the loop hands it a per-agent length
 *       array the mark launch wrote (e for a line-held agent, path_len[q] for everybody else) in place of path_len.  The goal test, the
 *       run log and prev_len (the next conflict search's prev_cut_len, restored by the clamp launch) stay the whole path's.
 *   (b) every entry t of row 2 of q's xref becomes fmin(entry, sqrt(2 brake d_t)), d_t the Euclidean distance of window point t (rows 0, 1)
 *       to E.  With advice and the following clamp on, all clamps apply; a minimum of minima does not depend on their order.
 *   (c) q is behind its line iff (x - p_s.x)(p_s.x - p_{s-1}.x) + (y - p_s.y)(p_s.y - p_{s-1}.y) < 0.  Behind: traj_idx[q] =
 *       min(traj_idx[q], e - 1), written after the holds have read traj_idx.  Not behind (a physical overrun): nothing is pinned, the hold
 *       frees the agent as it does without the stage, overran[q] += 1.
 *   (d) firm[q] = e, brake_cap[q] = the profile at window point 0.  An agent that is not line-held: firm = 0, brake_cap = 0.0, and nothing
 *       else of it is touched -- the window stage computes for it what it computes without the stage.
 * In MPCX_STOP_CUT the mark launch alone runs and writes firm and brake_cap = 0.0; nothing else changes, the cut is hard already.
 * NULL or an all-zero struct: off -- the loop enqueues exactly the launches of a context that never had it, with the same arguments.  The
 * cached graph's key covers the struct by value (two doubles and three pointers: 40 bytes, no padding), and a run with the stage on does
 * not take step fusion.  MPCX_E_INVALID ("braking: ...") from the run or a stage call before anything is launched, whatever n_steps is:
 * firm, overran or brake_cap NULL; brake not finite or not positive; setback not finite or below 2 dl (the pin needs two points between
 * e and s); the agent-sharded layout; more than one linearisation pass; a run with no source of stop lines (no signals, actuation,
 * reservation, priority road or stop signs). */
typedef struct {
    double brake;                /* m/s^2, > 0: the deceleration of the braking profile */
    double setback;              /* m, >= 2 dl: the stop point lies ceil(setback / dl) path points in front of the line */
    int32_t *firm;               /* P, caller-owned, out: 0, or the stop index e of a line-held agent */
    int32_t *overran;            /* P, caller-owned, in-out, zero-initialised: steps in which the agent was line-held beyond its line */
    double *brake_cap;           /* P, caller-owned, out: the braking profile at window point 0, 0.0 = not line-held (or MPCX_STOP_CUT) */
} mpcx_braking;
/* copies the struct into the context (the buffers it names stay the caller's and must stay valid while set); NULL or all-zero = off */
int32_t mpcx_set_braking(mpcx_ctx *ctx, const mpcx_braking *braking /*NULL or all-zero = off*/);
/* one step's mark launch alone (what the closed loop enqueues in front of the window stage).  held, boxed, yielding: the hold words that
 * are on (at least one).  MPCX_STOP_SPEED: target_ind is clamped and win_len written (both required); MPCX_STOP_CUT: both may be NULL. */
int32_t mpcx_brake_mark_step_batch(mpcx_ctx *ctx, int32_t P, double dl, int32_t stop_mode, const int32_t *path_off /*P*/,
                                   const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/, int32_t *target_ind /*P*/,
                                   int32_t *win_len /*P, out*/, const int32_t *done /*P or NULL*/, const int32_t *path_stop /*n_points*/,
                                   int32_t n_points, const int32_t *held /*P or NULL*/, const int32_t *boxed /*P or NULL*/,
                                   const int32_t *yielding /*P or NULL*/, const mpcx_braking *braking);
/* one step's clamp launch alone (what the closed loop enqueues behind every window stage in MPCX_STOP_SPEED): (b) - (d) on xref (P,4,T+1)
 * from firm as the mark launch left it.  prev_len: the words the window stage left at the window's length, or NULL. */
int32_t mpcx_brake_clamp_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state /*P,4*/, const double *path_xyyaw,
                                    const int32_t *path_off /*P*/, const int32_t *path_len /*P*/, int32_t *traj_idx /*P*/,
                                    int32_t *prev_len /*P or NULL*/, const int32_t *done /*P or NULL*/, const int32_t *path_stop /*n_points*/,
                                    int32_t n_points, const mpcx_braking *braking, double *xref /*P,4,T+1*/);

/* ---- the stages together.  With several optional stages on, a step is: admission, the entry-order stamp; pool pack and prediction; the
 * intent stage; the sight stage; the conflict search; the safety stage; the hold (signal, actuated or reserve stage); the keep-clear stage; the priority stage or the stop-sign stage (in the hold's place: never beside one, nor beside each other); the following stage; the firm hold's mark; per linearisation
 * pass the window stage, the advice stage, the following clamp, the firm hold's clamp and the QP; the plant; record, retire, respawn.  What that order implies:
 *   one car, three views   agent q sees a present row r of its window (1) standing at its pose if prec[r] > prec[obs_skip[q]], whatever
 *                          the intent stage wrote into r's predicted frames; (2) else on its owner's plan of the step before, if the owner
 *                          shares, drives, is present and its last status is MPCX_QP_OPTIMAL; (3) else through the constant prediction.
 *                          The following stage reads obs6[r] itself: the leader's true speed, whether it yields or shares.
 *   the cut is a minimum   conflict search, hold and follower each only lower cut_len; the advice stage reads the result.  A reservation
 *                          manager reads traj_idx as the conflict search left it and never the follower's stop point.
 *   a reset slot           the respawn stages reset no word of the signal, reservation, following or intent stages, nor status.  Each of
 *                          those stages rewrites its words for every agent in every step, retired ones included; a slot that is admitted
 *                          again in the very next step starts from what its predecessor's last step left (held, granted, since), and its
 *                          signal clock runs on.  Nor do they reset a word of the safety stage: tick, enc_row and n_events run on and
 *                          a slot's event table holds the events of every vehicle it carried; an event carries its ticks and path_off,
 *                          which is enough to join it with the episode table on the host.
 *   the safety stage       reads the prediction exactly as the conflict search read it and traj_idx as it left it; it writes no word any
 *                          other stage reads.
 *   the sight stage        only the conflict search reads its word.  The following stage and the near-miss log keep reading the physical
 *                          scene: a leader on one's own path is in view, and the log must see the contacts that occlusion causes (its
 *                          clearance is unchanged by construction).  Nor do the admission gate, the reservation manager or the run log's
 *                          clearance consult it.  A yielding row (precedence) or a sharing row (intent) that is not seen is simply not in
 *                          the agent's list.
 *   the keep-clear stage   reads held as this step's hold left it and never writes it: snapshot()'s held, the actuated controller's calls
 *                          and the advice stage see the lights alone.  It is one more minimum on cut_len, in front of the follower's.  It
 *                          reads traj_idx as the conflict search left it, like the reservation manager.  The respawn stages reset neither
 *                          boxed nor waited: a vehicle that arrives has been OUT since its exit point, and a reset slot waits at the
 *                          gate with done != 0, which is OUT too, so the stage itself has cleared waited before the slot's next
 *                          vehicle drives -- the word heals itself.
 *   the priority stage     reads traj_idx as the conflict search left it and the physical scene -- not the sight word, not prec: scripted
 *                          actors are members of no junction, and conflicts between equal ranks stay with the conflict search.  It is one
 *                          more minimum on cut_len, in front of the follower's.  A major-road car still reads an approaching minor car's
 *                          constant-velocity prediction and may brake for a car that is about to stop (give_way(order=) with the ranks
 *                          as words, or shared plans, are the remedies).  waited heals itself as keep clear's does: a reset slot is OUT
 *                          while it waits at the gate.  In MPCX_STOP_SPEED the hold is soft, as the signals' is.
 *   the stop-sign stage    reads traj_idx as the conflict search left it and the physical scene, like the priority stage, and is one more
 *                          minimum on cut_len in front of the follower's.  An unsigned car still reads a signed car's constant-velocity
 *                          prediction and may brake for a car that is about to stop.  go, stopped_at, stopping, lag and blocker heal
 *                          themselves: a reset slot is OUT while it waits at the gate; clock and ran run on.  In MPCX_STOP_SPEED the hold
 *                          is soft unless the firm hold is on: the path index of a standing car climbs to its line, the stage then sees
 *                          it INSIDE, and ran counts it.
 *   the firm hold          reads the hold words and traj_idx as this step's holds left them, and pins traj_idx only behind the last
 *                          launch that reads it.  It never touches cut_len: a conflict cut or a follower's stop point below the line keeps
 *                          zeroing the speed reference where it did.  Conflict-search stops are a moving stop index, not a line, and stay
 *                          soft; a boxed or yielding car has no patience.
 * tests/stack_helpers.py composes the host builds of the rules in this order; tests/test_gpu_stack.py replays the device against it. */
/* one step's search stage alone (what the closed loop enqueues in front of the window stage): steps 1 - 5.  stop_mode: MPCX_STOP_CUT or
 * MPCX_STOP_SPEED; the struct is the argument's, not the context's, and is checked as above. */
int32_t mpcx_follow_step_batch(mpcx_ctx *ctx, int32_t P, double dl, int32_t stop_mode, const double *state /*P,4*/, const double *path_xyyaw,
                               const int32_t *path_off /*P*/, const int32_t *path_len /*P*/, const int32_t *traj_idx /*P*/,
                               int32_t *cut_len /*P*/, const int32_t *done /*P or NULL*/, int32_t n_obs_pool, const double *obs6 /*NOBS,6*/,
                               const int32_t *obs_off /*P*/, const int32_t *obs_cnt /*P*/, const int32_t *obs_skip /*P or NULL*/,
                               const int32_t *absent /*NOBS or NULL*/, const mpcx_following *following);
/* one step's clamp alone (what the closed loop enqueues behind every window stage in MPCX_STOP_SPEED): step 6 on xref (P,4,T+1) from the
 * struct's cap as the search stage left it. */
int32_t mpcx_follow_cap_step_batch(mpcx_ctx *ctx, int32_t P, const int32_t *done /*P or NULL*/, const mpcx_following *following,
                                   double *xref /*P,4,T+1*/);

/* ---- multi-GPU exchange (the reference is single-process and has no counterpart).  One process per
 * GPU, one communicator per context: rank 0 calls mpcx_comm_unique_id, the caller distributes the MPCX_COMM_ID_BYTES bytes
 * to every rank by whatever means it has (torch.distributed broadcast in this package), every rank calls mpcx_comm_init.
 * mpcx_allgather_states is ONE RCCL all-gather over xGMI of 6-double agent states (x, y, v, yaw, accel, steer), enqueued on
 * the context's stream:
 *   MPCX_SHARD_INSTANCES  rank r holds n_inst instances x agents_local (= all) agents; all = the rank blocks one after the other
 *                         ([world * n_inst][agents_local][6]).  The instance-sharded data path itself needs no exchange
 *                         (all agents of an instance are rank-local); this form serves logging / result collection.
 *   MPCX_SHARD_AGENTS     rank r holds agents r*agents_local .. of EVERY one of n_inst instances; all = [n_inst][world *
 *                         agents_local][6], the obstacle pool of mpcx_interaction_batch on every rank (obs_off[p] = instance *
 *                         world * agents_local, obs_cnt[p] = world * agents_local, obs_skip[p] = the agent's own row).
 * Without a communicator (single rank) the call is a device copy.  local and all are DEVICE pointers. */
#define MPCX_COMM_ID_BYTES 128
#define MPCX_SHARD_INSTANCES 1
#define MPCX_SHARD_AGENTS 2
int32_t mpcx_comm_unique_id(void *id /*MPCX_COMM_ID_BYTES, host*/);
int32_t mpcx_comm_init(mpcx_ctx *ctx, int32_t world, int32_t rank, const void *id /*MPCX_COMM_ID_BYTES, host*/);
int32_t mpcx_comm_destroy(mpcx_ctx *ctx);
int32_t mpcx_allgather_states(mpcx_ctx *ctx, int32_t layout, int32_t n_inst, int32_t agents_local,
                              const double *local /*n_inst,agents_local,6*/, double *all /*see layout*/);

/* ---- scheduling hint for the next mpcx_qp_solve_batch calls (results never depend on it).  Interior-point iteration counts
 * are 5 for most problems with a tail to ~17, and one late-drawn hard problem ends the launch alone, so the work queue is
 * sorted longest-expected-first (counting sort, 64 bins) by
 *     key[b] = prev_iters[b]  (+ 6 if ref_now[b] != ref_prev[b]),
 * prev_iters = iterations problem b took in the previous MPC step (correlation with this step ~0.5), ref_now / ref_prev = any
 * pair of int32 arrays whose inequality marks a discontinuous change of the problem's reference since then -- the closed loop
 * passes the cut lengths of the current and the previous step (problems whose path cut moved take 8.0 iterations on average,
 * the others 5.3).  List-scheduling on recorded counts: ideal 28.7 rounds, FIFO 42-44, this order 31-32.  DEVICE pointers,
 * read at the start of each solve (prev_iters may alias the `iters` output); each may be NULL; all NULL = FIFO.
 * mpcx_closed_loop_run applies the hint by itself. */
int32_t mpcx_qp_set_order_hint(mpcx_ctx *ctx, const int32_t *prev_iters /*B or NULL*/, const int32_t *ref_now /*B or NULL*/,
                               const int32_t *ref_prev /*B or NULL*/);

/* ---- which kernel solves the QP:
 *   0 = automatic: the stage-structured solver for batches of >= 11264 problems or T > 20 (throughput: 8 problems per
 *       wavefront, O(T) work per iteration), the condensed solver below that (latency: 0.1-0.3 ms per launch against a
 *       0.4-0.8 ms floor);
 *   1 = condensed (csrc/mpcx_qp.hip, one wavefront per problem, any T <= MPCX_T_MAX, not competitive beyond T = 20);
 *   2 = stage-structured (csrc/mpcx_qp_quad.hip, eight lanes per problem, any T <= MPCX_T_MAX).
 * Same problem, same iteration, same exit rules: the choice changes speed, not results.  Both are tested against the oracle at
 * every T in 1..MPCX_T_MAX: the stage-structured solver within 1e-9, the condensed one within 1e-9 up to T = 20 and 5e-6 above
 * (its 64 x 64 condensed system is the less accurate of the two there).  The environment variable MPCX_QP_KERNEL=wave|stage sets
 * the default of new contexts. */
int32_t mpcx_set_qp_solver(mpcx_ctx *ctx, int32_t which);

/* ---- measurement hook: while enabled, every mpcx_qp_solve_batch launch (direct or through mpcx_closed_loop_run
 * without a graph) is bracketed by a pair of HIP events on the context's stream.  mpcx_profile_qp_read waits for
 * the recorded launches, returns their summed duration and count, and clears the record.  mpcx_closed_loop_run refuses use_graph
 * while the hook is on (launches inside a replayed graph cannot be bracketed). */
int32_t mpcx_profile_qp(mpcx_ctx *ctx, int32_t enable);
int32_t mpcx_profile_qp_read(mpcx_ctx *ctx, double *total_ms, int32_t *launches);

/* ---- per-instance tuning: the quantities main/lib/mpc_sensitivity.py:150-163 re-reads from
 * config/mpc_config_sensitivity.json before every solve, as one row per problem, so that a whole sensitivity sweep
 * (scenarios/mpc_sensitivity_analysis.py: one closed loop per parameter set) runs as ONE batch.  While rows are set,
 * problem b of every mpcx_qp_solve_batch / mpcx_plant_step_batch / mpcx_closed_loop_run call takes these fields
 * from rows[b] instead of the context-wide parameter set -- the batch size must equal n_rows; everything else (T, dt, L, speed and
 * steering limits, R_end, tolerances) still comes from mpcx_set_mpc_params.  rows is a DEVICE pointer that must
 * stay valid while set; (NULL, 0) clears. */
typedef struct {
    double w_perp, w_para;
    double R[2], Rd[2], Q_v_yaw[2];
    double Qf[4];        /* ALREADY multiplied by T */
    double max_accel, max_decel, max_dsteer /* rad/s */;
    double reserved;
} mpcx_qp_tuning;        /* 16 doubles */
int32_t mpcx_set_instance_tuning(mpcx_ctx *ctx, const mpcx_qp_tuning *rows, int32_t n_rows);

#ifdef __cplusplus
}
#endif
#endif
