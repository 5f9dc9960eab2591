// mpcx_respawn.hip -- respawn in the device-resident closed loop: a departed agent's slot is reset for the next vehicle of its stream and
// handed back to the admission gate.  The rule is mpcx_respawn_core.h.  One launch, one lane per agent, the LAST of a step -- after
// retire_kernel, whose arrival (done[q] = 1, the own row absent) it turns into an episode record and a waiting agent.  A lane whose agent is
// driving leaves after loading done[q]; every access is to words of agent q only, so no lane reads what another lane of the launch writes.
// Everything that changes is device memory: the launch has no step argument and a replayed hipGraph respawns like a plain run.  No LDS, no
// scratch; in steady state almost every wavefront leaves as a whole after one load per lane.
#include "mpcx_common.h"
#include "mpcx_respawn_core.h"

namespace mpcx {

__global__ __launch_bounds__(64) void respawn_kernel(RespawnArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    if (a.done[q] == 0) return;             // driving
    (void)respawn_agent(a, q);
}

}  // namespace mpcx

// all-zero (or no) struct: "no respawn"
bool mpcx_respawn_absent(const mpcx_respawn *s) {
    return !s || (s->generations == 0 && s->reserved == 0 && !s->start_state && !s->start_idx && !s->due && !s->served && !s->ep_i32 && !s->ep_f64);
}

// the struct's own fields and what respawn needs of the run; never a GPU fault for a bad one
int32_t mpcx_respawn_validate(mpcx_ctx *ctx, const mpcx_respawn *s, const mpcx_admit *admit) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: null struct");
    if (!admit)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: respawn needs admission (mpcx_admit, and with it mpcx_scene and mpcx_retire): a reset slot is a waiting agent, and the gate lets the next vehicle in");
    if (s->generations < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: generations = %d, at least one vehicle per slot", s->generations);
    const char *missing = !s->start_state ? "start_state" : !s->start_idx ? "start_idx" : !s->due ? "due" : !s->served ? "served" :
                          !s->ep_i32 ? "ep_i32" : !s->ep_f64 ? "ep_f64" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: start_state (P,4), start_idx (P), due (P,G), served (P), ep_i32 (P,G,8) and ep_f64 (P,G,2) are all required, %s is null", missing);
    return MPCX_OK;
}

// the launch alone (the structs have been checked): what the closed loop enqueues, also inside a capture
int32_t mpcx_respawn_enqueue(mpcx_ctx *ctx, int32_t P, double *state, double *applied, double *u_sol, int32_t *traj_idx, int32_t *target_ind,
                             int32_t *cut_len, int32_t *iters, int32_t *prev_len, const int32_t *obs_skip, int32_t n_obs_pool,
                             const mpcx_run_log *log, const mpcx_retire *retire, const mpcx_admit *admit, const mpcx_respawn *respawn) {
    mpcx::RespawnArgs a = {};
    a.P = P; a.n_pool = n_obs_pool; a.u_len = 2 * ctx->mpc.T;
    a.has_log = log ? 1 : 0; a.has_prev_len = prev_len ? 1 : 0;
    a.state = state; a.applied = applied; a.u_sol = u_sol;
    a.traj_idx = traj_idx; a.target_ind = target_ind; a.cut_len = cut_len; a.iters = iters; a.prev_len = prev_len;
    a.own_row = obs_skip;
    a.done = retire->done; a.steps_driven = retire->steps_driven;
    a.ad = *admit;
    if (log) a.log = *log;
    a.rs = *respawn;
    hipLaunchKernelGGL(mpcx::respawn_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "respawn_kernel");
}

extern "C" int32_t mpcx_respawn_step_batch(mpcx_ctx *ctx, int32_t P, double *state, double *applied, double *u_sol, int32_t *traj_idx,
                                           int32_t *target_ind, int32_t *cut_len, int32_t *iters, int32_t *prev_len, const int32_t *obs_skip,
                                           int32_t n_obs_pool, const mpcx_run_log *log, const mpcx_retire *retire, const mpcx_admit *admit,
                                           const mpcx_respawn *respawn) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (P < 0 || n_obs_pool < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "respawn_step_batch: negative size");
    if (!respawn) return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: null struct");
    if (!admit || !admit->wait || !admit->entered_step || !admit->clock)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: respawn needs admission (mpcx_admit with wait, entered_step and clock)");
    if (!retire || !retire->done || !retire->steps_driven)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: respawn needs retirement (mpcx_retire with done and steps_driven)");
    int32_t rc = mpcx_respawn_validate(ctx, respawn, admit);
    if (rc != MPCX_OK) return rc;
    if (mpcx_record_absent(log)) log = nullptr;
    if (log) {
        rc = mpcx_record_validate(ctx, log, obs_skip);
        if (rc != MPCX_OK) return rc;
    }
    if (!state || !applied || !u_sol || !traj_idx || !target_ind || !cut_len || !iters || !obs_skip)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn_step_batch: null buffer (state, applied, u_sol, traj_idx, target_ind, cut_len, iters, obs_skip)");
    if (P == 0) return MPCX_OK;
    return mpcx_respawn_enqueue(ctx, P, state, applied, u_sol, traj_idx, target_ind, cut_len, iters, prev_len, obs_skip, n_obs_pool, log, retire,
                                admit, respawn);
}
