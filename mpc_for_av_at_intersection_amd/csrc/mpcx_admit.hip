// mpcx_admit.hip -- admission in the device-resident closed loop: agents enter the scene on a schedule (the counterpart of departure).  The
// rule is mpcx_admit_core.h.  Two launches, the FIRST of a step -- before the rollout is forked, which already reads done[], so that every
// stage of the step sees an admitted agent as driving and present:
//   admit_snapshot_kernel   one lane per agent and per scripted actor: the pose the step's pool will hold for its row and the row's tag
//                           into the context's table; lane 0 advances the clock
//   admit_gate_kernel       one lane per agent: count a waiting agent down, judge a due one from the table alone
// No lane reads a word another lane of the same launch writes.  Everything that changes is device memory, so the launches have no step
// argument and a replayed hipGraph admits agents like a plain run.  No LDS; in steady state nobody is due and the gate is one load per lane.
#include "mpcx_common.h"
#include "mpcx_admit_core.h"
#include <cmath>

namespace mpcx {

__global__ __launch_bounds__(64) void admit_snapshot_kernel(AdmitArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) admit_tick(a);
    if (i < a.P) admit_snapshot_agent(a, i);
    else if (i - a.P < a.n_actors) admit_snapshot_actor(a, i - a.P);
}

__global__ __launch_bounds__(64) void admit_gate_kernel(AdmitArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    if (a.ad.wait[q] < 0) return;           // not scheduled, or in already: almost every wavefront leaves here as a whole
    (void)admit_gate_agent(a, q);
}

}  // namespace mpcx

// all-zero (or no) struct: "no admission"
bool mpcx_admit_absent(const mpcx_admit *a) {
    return !a || (!a->wait && !a->entered_step && !a->clock && a->reserved == 0 && a->gap == 0.0);
}

// the struct's own fields and what admission needs of the run; never a GPU fault for a bad one
int32_t mpcx_admit_validate(mpcx_ctx *ctx, const mpcx_admit *a, const mpcx_retire *retire, const mpcx_scene *scene, int32_t exchange) {
    if (!a) return mpcx_fail(ctx, MPCX_E_INVALID, "admit: null struct");
    if (!scene || !retire)
        return mpcx_fail(ctx, MPCX_E_INVALID, "admit: admission needs a scene (mpcx_scene, and with it mpcx_retire): a waiting agent is a retired one whose own row is absent");
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "admit: not supported in the agent-sharded layout (a remote rank's mask would have to travel with the all-gather)");
    if (!a->wait || !a->entered_step || !a->clock)
        return mpcx_fail(ctx, MPCX_E_INVALID, "admit: wait, entered_step (P int32 each) and clock (1 int32) are all required, %s is null",
                         !a->wait ? "wait" : !a->entered_step ? "entered_step" : "clock");
    if (!std::isfinite(a->gap) || a->gap < 0.0) return mpcx_fail(ctx, MPCX_E_INVALID, "admit: gap must be finite and >= 0");
    return MPCX_OK;
}

// the table for a pool of n_rows: [n_rows][3] poses | [n_rows] tags.  Grown outside any capture; the tags are cleared once per call of an
// entry point, so that a row nobody owns (which no snapshot lane writes) is nobody
int32_t mpcx_admit_prepare(mpcx_ctx *ctx, size_t n_rows) {
    const int32_t rc = mpcx_grow(ctx, (void **)&ctx->admit_tab, &ctx->admit_tab_cap, n_rows * (3 * sizeof(double) + sizeof(int32_t)), "the admission table");
    if (rc != MPCX_OK || n_rows == 0) return rc;
    if (hipMemsetAsync(ctx->admit_tab + 3 * n_rows, 0, n_rows * sizeof(int32_t), ctx->stream) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "admit: hipMemsetAsync failed");
    return MPCX_OK;
}

// the two launches alone (struct checked, table prepared): what the closed loop enqueues, also inside a capture
int32_t mpcx_admit_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *obs_off,
                           const int32_t *obs_cnt, const int32_t *obs_skip, int32_t *done, int32_t n_obs_pool, int32_t *absent,
                           int32_t n_actors, const mpcx_traffic_actor *actors, const double *actor_state, const double *tape,
                           int64_t tape_rows, const int32_t *actor_row, const mpcx_admit *admit) {
    mpcx::AdmitArgs a;
    a.P = P; a.n_pool = n_obs_pool; a.n_actors = n_actors;
    a.radius = ip->radius;
    for (int k = 0; k < 4; k++) a.cc[k] = ip->circle_centers[k];
    a.state = state; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.own_row = obs_skip;
    a.done = done; a.absent = absent;
    a.actors = actors; a.actor_state = actor_state; a.tape = tape; a.tape_rows = tape ? tape_rows : (int64_t)0; a.actor_row = actor_row;
    a.ad = *admit;
    a.tab_pose = ctx->admit_tab;
    a.tab_tag = reinterpret_cast<int32_t *>(ctx->admit_tab + 3 * (size_t)n_obs_pool);
    hipLaunchKernelGGL(mpcx::admit_snapshot_kernel, dim3((P + n_actors + 63) / 64), dim3(64), 0, ctx->stream, a);
    int32_t rc = mpcx_check_launch(ctx, "admit_snapshot_kernel");
    if (rc != MPCX_OK) return rc;
    hipLaunchKernelGGL(mpcx::admit_gate_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "admit_gate_kernel");
}

extern "C" int32_t mpcx_admit_step_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *obs_off,
                                         const int32_t *obs_cnt, const int32_t *obs_skip, int32_t *done, int32_t n_obs_pool, int32_t *absent,
                                         int32_t n_actors, const mpcx_traffic_actor *actors, const double *actor_state, const double *tape,
                                         int64_t tape_rows, const int32_t *actor_row, const mpcx_admit *admit) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ip || P < 0 || n_obs_pool < 0 || n_actors < 0 || tape_rows < 0)
        return mpcx_fail(ctx, MPCX_E_INVALID, "admit_step_batch: null parameters or negative size");
    if (!admit) return mpcx_fail(ctx, MPCX_E_INVALID, "admit: null struct");
    if (!admit->wait || !admit->entered_step || !admit->clock)
        return mpcx_fail(ctx, MPCX_E_INVALID, "admit: wait, entered_step (P int32 each) and clock (1 int32) are all required, %s is null",
                         !admit->wait ? "wait" : !admit->entered_step ? "entered_step" : "clock");
    if (!std::isfinite(admit->gap) || admit->gap < 0.0) return mpcx_fail(ctx, MPCX_E_INVALID, "admit: gap must be finite and >= 0");
    if (!state || !obs_off || !obs_cnt || !obs_skip || !done || !absent)
        return mpcx_fail(ctx, MPCX_E_INVALID, "admit_step_batch: null buffer (state, obs_off, obs_cnt, obs_skip, done, absent)");
    if (n_actors > 0) {
        if (!actors || !actor_state || !actor_row) return mpcx_fail(ctx, MPCX_E_INVALID, "admit_step_batch: scripted actors need actors, actor_state and actor_row");
        const int32_t trc = mpcx_traffic_validate(ctx, n_actors, actors, tape, tape_rows, actor_row, n_obs_pool);
        if (trc != MPCX_OK) return trc;
    }
    if (P == 0) return MPCX_OK;
    const int32_t rc = mpcx_admit_prepare(ctx, (size_t)n_obs_pool);
    if (rc != MPCX_OK) return rc;
    return mpcx_admit_enqueue(ctx, ip, P, state, obs_off, obs_cnt, obs_skip, done, n_obs_pool, absent, n_actors, actors, actor_state, tape,
                              tape_rows, actor_row, admit);
}
