// mpcx_interaction.hip -- ego-vs-moving-cars conflict search and reference-path cut, batched.
//
// Replaces (paths relative to /root/reference/main):
//   lib/moving_obstacles_prediction.py:21-47  MovingObstaclesPrediction.state_prediction -> predict_kernel
//   scenarios/mpc_intersection.py:103-116     nearest index on the full path + ego prediction resampling
//   lib/trajectories.py:58-86                 resample_curve (vector dl)
//   lib/collision_avoidance.py:66-104         check_collision_moving_cars
//   lib/collision_avoidance.py:107-119 + mpc_intersection.py:129-136  cut-off index
// One wavefront per ego.  The reference flattens (frame, agent disc, obstacle x frame-offset, obstacle disc)
// into one pair table and takes the first row within 2*radius; here every obstacle disc position (<= 16*64*2,
// one global load each) is culled exactly against the bounding box of all ego discs and then against the boxes
// of 8 runs of ego frames, compared only with the frames of surviving runs that a +-frame_window shift can
// reach, and the FIRST ROW IN THE REFERENCE'S ORDER is recovered as the minimum of an integer key over all hits
// (bit-exact index outputs).
#include "mpcx_interaction_parts.h"

namespace mpcx {

// ------------------------------------------------------------------------------------------------------------
// check_collision_moving_cars on EXPLICIT trajectories (the reference's own signature, collision_avoidance.py:66):
// the caller has already resampled the ego and predicted the obstacles (mpc_intersection.py:110-122).
struct PoseDiscArgs {
    mpcx_interaction_params ip;
    int n;                       // number of poses
    const double *pose, *cs;     // [n][3] (x,y,yaw), [n][2] (cos,sin of yaw)
    double *out;                 // [n][4] disc centres
};
__global__ __launch_bounds__(256) void pose_disc_kernel(PoseDiscArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double px = a.pose[3 * i], py = a.pose[3 * i + 1], c = a.cs[2 * i], s = a.cs[2 * i + 1];
    pose_discs(a.ip, px, py, c, s, a.out + 4 * i);
}

struct MovArgs {
    mpcx_interaction_params ip;
    int P;
    const double *ego, *ego_cs;
    const int32_t *ego_off, *ego_len;
    const double *path, *path_cs;
    const int32_t *path_off, *path_len;
    const double *pred;
    const int32_t *obs_off, *obs_cnt;
    int32_t *hit_idx;
    double *hit_xy;
};

__global__ __launch_bounds__(64) void moving_collision_kernel(MovArgs a) {
    __shared__ double s_ego[MPCX_EGO_FRAMES_MAX][4];
    __shared__ double s_box[NSEG][4];
    const int p = blockIdx.x, lane = threadIdx.x;
    const mpcx_interaction_params &ip = a.ip;
    const int na = a.ego_len[p], n = a.path_len[p], nobs = a.obs_cnt[p];
    if (nobs <= 0) { if (lane == 0) { a.hit_idx[p] = -1; a.hit_xy[2 * p] = 0; a.hit_xy[2 * p + 1] = 0; } return; }
    if (na > MPCX_EGO_FRAMES_MAX || na < 1 || n < 1 || nobs > MPCX_MAX_OBS) { if (lane == 0) { a.hit_idx[p] = -2; a.hit_xy[2 * p] = 0; a.hit_xy[2 * p + 1] = 0; } return; }
    const double *ego = a.ego + 3 * (size_t)a.ego_off[p], *ecs = a.ego_cs + 2 * (size_t)a.ego_off[p];
    for (int f = lane; f < na; f += WAVE) {
        const double px = ego[3 * f], py = ego[3 * f + 1], c = ecs[2 * f], s = ecs[2 * f + 1];
        pose_discs(ip, px, py, c, s, s_ego[f]);
    }
    __syncthreads();
    double hx, hy;
    const int first = first_conflict(ip, s_ego, na, a.pred, a.obs_off[p], nobs, -1,
                                     a.path + 3 * (size_t)a.path_off[p], a.path_cs + 2 * (size_t)a.path_off[p], n, s_box, lane, hx, hy);
    if (lane == 0) { a.hit_idx[p] = first; a.hit_xy[2 * p] = first < 0 ? 0.0 : hx; a.hit_xy[2 * p + 1] = first < 0 ? 0.0 : hy; }
}

// One launcher per kernel: the instantiation follows from what the call carries -- right of way (x.prec; compiled in mpcx_interaction_prec.hip),
// line of sight (x.sight; compiled in mpcx_interaction_sight.hip), a scene (x.absent), retirement (x.done) or none of them.
static void launch_predict(bool mapped, int lanes, hipStream_t st, const PredArgs &pa, const mpcx_interaction_extras &x) {
    const dim3 grid((lanes + 63) / 64), block(64);
    if (x.prec) launch_predict_stand(mapped, lanes, st, pa);
    else if (mapped && x.absent) hipLaunchKernelGGL((predict_kernel<true, true>), grid, block, 0, st, pa);
    else if (mapped) hipLaunchKernelGGL(predict_kernel<true>, grid, block, 0, st, pa);
    else if (x.absent) hipLaunchKernelGGL((predict_kernel<false, true>), grid, block, 0, st, pa);
    else hipLaunchKernelGGL(predict_kernel<false>, grid, block, 0, st, pa);
}

static void launch_interaction(int P, size_t lds, hipStream_t st, const InterArgs &ia, const mpcx_interaction_extras &x) {
    if (x.sight) launch_interaction_sight(P, lds, st, ia, (const unsigned long long *)x.sight->sight, x.prec != nullptr);
    else if (x.prec) launch_interaction_prec(P, lds, st, ia);
    else if (x.absent) hipLaunchKernelGGL((interaction_kernel<true, true>), dim3(P), dim3(64), lds, st, ia);
    else if (x.done) hipLaunchKernelGGL(interaction_kernel<true>, dim3(P), dim3(64), lds, st, ia);
    else hipLaunchKernelGGL(interaction_kernel<false>, dim3(P), dim3(64), lds, st, ia);
}

}  // namespace mpcx

// The launch's path capacity: max_path_len path points (0 = MPCX_MAX_REMAINING; never below 512), rounded up to whole wavefronts.
int32_t mpcx_interaction_capacity(const mpcx_interaction_params *ip) {
    int32_t cap = ip->max_path_len > 0 ? ip->max_path_len : MPCX_MAX_REMAINING;
    if (cap < 512) cap = 512;
    return (cap + 63) / 64 * 64;
}

extern "C" int32_t mpcx_interaction_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                                          const double *state, const double *path_xyyaw, const double *path_cs,
                                          const int32_t *path_off, const int32_t *path_len, const int32_t *prev_cut_len,
                                          int32_t n_obs_pool, const double *obs6, const int32_t *obs_off,
                                          const int32_t *obs_cnt, const int32_t *obs_skip,
                                          int32_t *traj_idx, int32_t *hit_idx, double *hit_xy, int32_t *cut_len) {
    return mpcx_interaction_enqueue(ctx, ip, P, state, path_xyyaw, path_cs, path_off, path_len, prev_cut_len, n_obs_pool, obs6, obs_off,
                                    obs_cnt, obs_skip, traj_idx, hit_idx, hit_xy, cut_len, {});
}

int32_t mpcx_interaction_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const double *path_xyyaw,
                                 const double *path_cs, const int32_t *path_off, const int32_t *path_len, const int32_t *prev_cut_len,
                                 int32_t n_obs_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip,
                                 int32_t *traj_idx, int32_t *hit_idx, double *hit_xy, int32_t *cut_len, const mpcx_interaction_extras &x) {
    if (!ctx) return MPCX_E_INVALID;
    if (P == 0) return MPCX_OK;
    if (!ip || P < 0 || n_obs_pool < 0 || !state || !path_xyyaw || !path_cs || !path_off || !path_len || !obs_off ||
        !obs_cnt || !traj_idx || !hit_idx || !hit_xy || !cut_len || (n_obs_pool > 0 && !obs6))
        return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch: null pointer or negative size");
    if (ip->pred_steps < 1 || ip->pred_steps > MPCX_PRED_STEPS_MAX || ip->frame_window < 0 || !(ip->dt > 0) || !(ip->L > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch: pred_steps outside 1..%d or bad dt/L/frame_window", MPCX_PRED_STEPS_MAX);
    if (x.absent && (!x.done || n_obs_pool < 1)) return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch: a scene without retirement or without a pool");
    if ((x.prec || x.stand) && (!x.absent || !x.prec || !x.stand)) return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch: precedence without a scene, or without one of prec and stand");
    if (x.sight && (!x.absent || !obs_skip)) return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch: line of sight without a scene or without obs_skip");
    { int32_t rc = mpcx_ensure_pred(ctx, (size_t)(n_obs_pool > 0 ? n_obs_pool : 1) * ip->pred_steps * 4); if (rc != MPCX_OK) return rc; }
    if (x.predicted) {
        // (the head of the closed loop's step has packed and predicted the pool already)
    } else if (n_obs_pool > 0 && x.pack_state && x.ego_row) {
        // closed loop with scripted traffic: only the rows that hold an agent or an actor are predicted (the others are outside every window)
        const int lanes = x.n_ego + x.n_actors;
        mpcx::PredArgs pa{*ip, lanes, n_obs_pool, obs6, ctx->pred, x.pack_state, x.pack_applied, const_cast<double *>(obs6),
                          x.ego_row, x.actor_row, x.n_ego, x.absent, x.stand};
        mpcx::launch_predict(true, lanes, ctx->stream, pa, x);
    } else if (n_obs_pool > 0) {
        mpcx::PredArgs pa{*ip, n_obs_pool, n_obs_pool, obs6, ctx->pred, x.pack_state, x.pack_applied, x.pack_state ? const_cast<double *>(obs6) : nullptr,
                          nullptr, nullptr, 0, x.absent, x.stand};
        mpcx::launch_predict(false, n_obs_pool, ctx->stream, pa, x);
    }
    if (x.intent) {     // shared plans: the sharing agents' own rows are re-rolled from their plans before anybody searches them
        const int32_t rc = mpcx_intent_enqueue(ctx, ip, P, state, obs_skip, n_obs_pool, *x.intent);
        if (rc != MPCX_OK) return rc;
    }
    if (x.sight) {      // line of sight: every agent's word of seen rows, on the pool as packed, before anybody searches it
        const int32_t rc = mpcx_sight_enqueue(ctx, P, state, x.done, n_obs_pool, obs6, obs_off, obs_cnt, obs_skip, x.absent, x.sight);
        if (rc != MPCX_OK) return rc;
    }
    // capacity (mpcx_interaction_capacity): the LDS that holds the cumulative lengths of max_rem path points later holds the ego discs of
    // max_rem / 4 - 32 resampled poses and the runs' boxes.
    // The kernel hides its memory latency with resident wavefronts (17 -> 11 blocks per CU costs 36 %), so the LDS follows the
    // call's longest path instead of a fixed 1024 points.
    const int max_rem = mpcx_interaction_capacity(ip);
    if (max_rem > MPCX_MAX_PATH_LEN)
        return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch: max_path_len %d exceeds %d", ip->max_path_len, MPCX_MAX_PATH_LEN);
    const int fcap = max_rem / 4 - mpcx::SPARE_ROWS;
    const size_t lds = (size_t)max_rem * sizeof(double) + ((size_t)fcap * sizeof(unsigned short) + 7) / 8 * 8;
    mpcx::InterArgs ia{*ip, P, state, path_xyyaw, path_cs, path_off, path_len, prev_cut_len, ctx->pred,
                       obs_off, obs_cnt, obs_skip, traj_idx, hit_idx, hit_xy, cut_len, max_rem, fcap, x.prev_save,
                       x.bin_hint, x.bin_hint ? ctx->bins : nullptr, x.bin_hint ? ctx->bins + MPCX_ORDER_COPIES * MPCX_ORDER_BINS : nullptr,
                       x.key_prev, x.near, x.done, x.absent, n_obs_pool, x.prec, x.stand};
    mpcx::launch_interaction(P, lds, ctx->stream, ia, x);
    return mpcx_check_launch(ctx, "interaction kernels");
}

int32_t mpcx_ensure_pred(mpcx_ctx *ctx, size_t need) {
    return mpcx_grow(ctx, (void **)&ctx->pred, &ctx->pred_cap, need * sizeof(double), "the prediction scratch");
}

extern "C" int32_t mpcx_interaction_prediction(mpcx_ctx *ctx, int32_t rows, int32_t steps, double *out) {
    if (!ctx || !out || rows < 0 || steps < 1 || steps > MPCX_PRED_STEPS_MAX) return MPCX_E_INVALID;
    const size_t bytes = (size_t)rows * steps * 4 * sizeof(double);
    if (!ctx->pred || ctx->pred_cap < bytes)
        return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_prediction: no prediction of %d rows x %d frames has been made on this context", rows, steps);
    if (rows == 0) return MPCX_OK;
    if (hipMemcpyAsync(out, ctx->pred, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "interaction_prediction: copy failed");
    return MPCX_OK;
}

extern "C" int32_t mpcx_moving_collision_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P,
                                               const double *ego_xyyaw, const double *ego_cs, const int32_t *ego_off,
                                               const int32_t *ego_len, const double *path_xyyaw, const double *path_cs,
                                               const int32_t *path_off, const int32_t *path_len,
                                               int32_t n_obs_pool, const double *obs_xyyaw, const double *obs_cs,
                                               const int32_t *obs_off, const int32_t *obs_cnt,
                                               int32_t *hit_idx, double *hit_xy) {
    if (!ctx) return MPCX_E_INVALID;
    if (P == 0) return MPCX_OK;
    if (!ip || P < 0 || n_obs_pool < 0 || !ego_xyyaw || !ego_cs || !ego_off || !ego_len || !path_xyyaw || !path_cs ||
        !path_off || !path_len || !obs_off || !obs_cnt || !hit_idx || !hit_xy || (n_obs_pool > 0 && (!obs_xyyaw || !obs_cs)))
        return mpcx_fail(ctx, MPCX_E_INVALID, "moving_collision_batch: null pointer or negative size");
    if (ip->pred_steps < 1 || ip->pred_steps > MPCX_PRED_STEPS_MAX || ip->frame_window < 0)
        return mpcx_fail(ctx, MPCX_E_INVALID, "moving_collision_batch: pred_steps outside 1..%d or negative frame_window", MPCX_PRED_STEPS_MAX);
    const size_t nposes = (size_t)n_obs_pool * ip->pred_steps;
    int32_t rc = mpcx_ensure_pred(ctx, (nposes ? nposes : 1) * 4);
    if (rc != MPCX_OK) return rc;
    if (nposes) {
        mpcx::PoseDiscArgs pd{*ip, (int)nposes, obs_xyyaw, obs_cs, ctx->pred};
        hipLaunchKernelGGL(mpcx::pose_disc_kernel, dim3((unsigned)((nposes + 255) / 256)), dim3(256), 0, ctx->stream, pd);
    }
    mpcx::MovArgs ma{*ip, P, ego_xyyaw, ego_cs, ego_off, ego_len, path_xyyaw, path_cs, path_off, path_len, ctx->pred,
                     obs_off, obs_cnt, hit_idx, hit_xy};
    hipLaunchKernelGGL(mpcx::moving_collision_kernel, dim3(P), dim3(64), 0, ctx->stream, ma);
    return mpcx_check_launch(ctx, "moving collision kernels");
}
