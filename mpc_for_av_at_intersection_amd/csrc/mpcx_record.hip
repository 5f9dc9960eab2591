// mpcx_record.hip -- the run log of the device-resident closed loop: what the reference's loop produces ABOUT a run (HistorySimulation's
// rows, main/lib/simulation.py:58-88; the end of the loop, mpc.is_goal, main/lib/mpc.py:310-326) and the true distance between the
// vehicles.  One lane per agent, one launch per step, last in the step (after plant_kernel): evaluate the record rule
// (mpcx_record_core.h), write the agent's row.  All mutable state -- the write cursor included -- is device memory, so the launch has no
// step argument and a replayed hipGraph keeps advancing.
// Rows are laid out [step][agent][8]: a wavefront writes 4 KB of doubles and 2 KB of integers, each contiguous, as 16-byte stores.
#include "mpcx_common.h"
#include "mpcx_record_core.h"

namespace mpcx {

__global__ __launch_bounds__(64) void record_kernel(RecordArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    if (a.done && a.done[q] != 0) return;   // retired at the goal: no row, cursor and outcome words stay
    double f[REC_F64];
    int32_t w[REC_I32];
    const int32_t s = record_agent(a, q, f, w);
    if (s >= a.log.capacity) return;        // (capacity 0: the row pointers are never touched)
    const size_t row = (size_t)s * (size_t)a.P + (size_t)q;
    double2 *df = reinterpret_cast<double2 *>(a.log.rows_f64 + REC_F64 * row);
#pragma unroll
    for (int k = 0; k < REC_F64 / 2; k++) df[k] = make_double2(f[2 * k], f[2 * k + 1]);
    int4 *di = reinterpret_cast<int4 *>(a.log.rows_i32 + REC_I32 * row);
#pragma unroll
    for (int k = 0; k < REC_I32 / 4; k++) di[k] = make_int4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

}  // namespace mpcx

// capacity 0 and every pointer NULL: "no log"
bool mpcx_record_absent(const mpcx_run_log *log) {
    return !log || (log->capacity == 0 && !log->rows_f64 && !log->rows_i32 && !log->steps && !log->goal_step && !log->contact_step &&
                    !log->flags && !log->min_clearance);
}

// the descriptor's own fields; never a GPU fault for a bad one
int32_t mpcx_record_validate(mpcx_ctx *ctx, const mpcx_run_log *log, const int32_t *obs_skip) {
    if (!log) return mpcx_fail(ctx, MPCX_E_INVALID, "run log: null descriptor");
    if (log->capacity < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "run log: negative capacity %d", log->capacity);
    if (log->capacity > 0 && (!log->rows_f64 || !log->rows_i32))
        return mpcx_fail(ctx, MPCX_E_INVALID, "run log: capacity %d and no row buffers (rows_f64 / rows_i32)", log->capacity);
    if (((uintptr_t)log->rows_f64 | (uintptr_t)log->rows_i32) & 15)
        return mpcx_fail(ctx, MPCX_E_INVALID, "run log: the row buffers must be 16-byte aligned");
    if (!log->steps || !log->goal_step || !log->contact_step || !log->flags || !log->min_clearance)
        return mpcx_fail(ctx, MPCX_E_INVALID, "run log: null outcome buffer (steps, goal_step, contact_step, flags, min_clearance)");
    if (!(log->goal_dis >= 0.0) || !(log->stop_speed >= 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "run log: goal_dis and stop_speed must be >= 0");
    if (!obs_skip) return mpcx_fail(ctx, MPCX_E_INVALID, "run log: obs_skip is required (the agent's own pool row is its pose for the clearance)");
    return MPCX_OK;
}

// the launch alone (the descriptor has been checked): what the closed loop enqueues, also inside a capture
int32_t mpcx_record_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const double *applied,
                            const double *x_sol, const double *path_xyyaw, const int32_t *path_off, const int32_t *path_len,
                            const int32_t *target_ind, const int32_t *cut_len, const int32_t *traj_idx, const int32_t *hit_idx,
                            const int32_t *status, const int32_t *iters, int32_t n_obs_pool, const double *obs6, const int32_t *obs_off,
                            const int32_t *obs_cnt, const int32_t *obs_skip, const mpcx_run_log *log, const int32_t *goal_len,
                            const int32_t *done, const int32_t *absent) {
    mpcx::RecordArgs a;
    a.P = P; a.n_pool = n_obs_pool;
    a.x_stride = 4 * (int64_t)(ctx->mpc.T + 1);
    a.radius = ip->radius;
    for (int k = 0; k < 4; k++) a.cc[k] = ip->circle_centers[k];
    a.state = state; a.applied = applied; a.x_sol = x_sol; a.path_xyyaw = path_xyyaw; a.obs6 = obs6;
    a.path_off = path_off; a.path_len = path_len; a.target_ind = target_ind; a.cut_len = cut_len; a.traj_idx = traj_idx;
    a.hit_idx = hit_idx; a.status = status; a.iters = iters;
    a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip;
    a.log = *log;
    a.goal_len = goal_len;
    a.done = done;
    a.absent = absent;
    hipLaunchKernelGGL(mpcx::record_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "record_kernel");
}

extern "C" int32_t mpcx_record_step_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state,
                                          const double *applied, const double *x_sol, const double *path_xyyaw, const int32_t *path_off,
                                          const int32_t *path_len, const int32_t *target_ind, const int32_t *cut_len,
                                          const int32_t *traj_idx, const int32_t *hit_idx, const int32_t *status, const int32_t *iters,
                                          int32_t n_obs_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt,
                                          const int32_t *obs_skip, const mpcx_run_log *log) {
    return mpcx_record_step_batch_goal(ctx, ip, P, state, applied, x_sol, path_xyyaw, path_off, path_len, target_ind, cut_len, traj_idx, hit_idx,
                                       status, iters, n_obs_pool, obs6, obs_off, obs_cnt, obs_skip, nullptr, log);
}

extern "C" int32_t mpcx_record_step_batch_goal(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state,
                                          const double *applied, const double *x_sol, const double *path_xyyaw, const int32_t *path_off,
                                          const int32_t *path_len, const int32_t *target_ind, const int32_t *cut_len,
                                          const int32_t *traj_idx, const int32_t *hit_idx, const int32_t *status, const int32_t *iters,
                                          int32_t n_obs_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt,
                                          const int32_t *obs_skip, const int32_t *goal_len, const mpcx_run_log *log) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (!ip || P < 0 || n_obs_pool < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "record_step_batch: null parameters or negative size");
    int32_t rc = mpcx_record_validate(ctx, log, obs_skip);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !applied || !x_sol || !path_xyyaw || !path_off || !path_len || !target_ind || !cut_len || !traj_idx || !hit_idx ||
        !status || !iters || !obs6 || !obs_off || !obs_cnt)
        return mpcx_fail(ctx, MPCX_E_INVALID, "record_step_batch: null buffer");
    return mpcx_record_enqueue(ctx, ip, P, state, applied, x_sol, path_xyyaw, path_off, path_len, target_ind, cut_len, traj_idx, hit_idx,
                               status, iters, n_obs_pool, obs6, obs_off, obs_cnt, obs_skip, log, goal_len);
}
