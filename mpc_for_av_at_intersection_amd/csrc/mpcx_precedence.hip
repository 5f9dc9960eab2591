// mpcx_precedence.hip -- right of way in the device-resident closed loop: the struct's checks and the entry-order stamp of
// MPCX_PRECEDENCE_ENTRY.  The rule of the stamp is mpcx_precedence_core.h; the rule the words stand for is applied by the PREC instantiations
// of predict_kernel and interaction_kernel (mpcx_interaction_parts.h; instantiated in mpcx_interaction_prec.hip).
// precedence_stamp_kernel: one launch right after the admission stage, one lane per agent, one store per agent in the scene.  No LDS, no
// scratch.  Everything it reads is device memory the step itself maintains, so a replayed hipGraph stamps like a plain run.
#include "mpcx_common.h"
#include "mpcx_precedence_core.h"

namespace mpcx {

__global__ __launch_bounds__(64) void precedence_stamp_kernel(StampArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    (void)precedence_stamp_agent(a, q);
}

}  // namespace mpcx

// all-zero (or no) struct: "no precedence"
bool mpcx_precedence_absent(const mpcx_precedence *s) {
    return !s || (!s->prec && !s->stand && s->n_rows == 0 && s->mode == 0);
}

// the struct's own fields and what precedence needs of the run; never a GPU fault for a bad one
int32_t mpcx_precedence_validate(mpcx_ctx *ctx, const mpcx_precedence *s, const mpcx_scene *scene, const mpcx_admit *admit) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "precedence: null struct");
    if (s->mode != MPCX_PRECEDENCE_FIXED && s->mode != MPCX_PRECEDENCE_ENTRY)
        return mpcx_fail(ctx, MPCX_E_INVALID, "precedence: unknown mode %d (MPCX_PRECEDENCE_FIXED or MPCX_PRECEDENCE_ENTRY)", s->mode);
    if (!scene)
        return mpcx_fail(ctx, MPCX_E_INVALID, "precedence: precedence needs a scene (mpcx_scene, and with it mpcx_retire): the yielding rows are found among the present rows of the window");
    if (!s->prec || !s->stand)
        return mpcx_fail(ctx, MPCX_E_INVALID, "precedence: prec (n_rows int32) and stand (n_rows x 4 doubles) are both required, %s is null", !s->prec ? "prec" : "stand");
    if (s->n_rows != scene->n_rows)
        return mpcx_fail(ctx, MPCX_E_INVALID, "precedence: n_rows = %d, the pool has %d rows", s->n_rows, scene->n_rows);
    if (s->mode == MPCX_PRECEDENCE_ENTRY && !admit)
        return mpcx_fail(ctx, MPCX_E_INVALID, "precedence: MPCX_PRECEDENCE_ENTRY needs admission (mpcx_admit): the order of entry is entered_step");
    return MPCX_OK;
}

// the launch alone (structs checked): what the closed loop enqueues after the admission stage in ENTRY mode, also inside a capture
int32_t mpcx_precedence_enqueue(mpcx_ctx *ctx, int32_t P, const int32_t *obs_off, const int32_t *obs_skip, const mpcx_admit *admit,
                                const mpcx_precedence *precedence) {
    const mpcx::StampArgs a{P, precedence->n_rows, obs_off, obs_skip, admit->entered_step, precedence->prec};
    hipLaunchKernelGGL(mpcx::precedence_stamp_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "precedence_stamp_kernel");
}

extern "C" int32_t mpcx_admit_step_batch_precedence(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state,
                                                    const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip, int32_t *done,
                                                    int32_t n_obs_pool, int32_t *absent, int32_t n_actors, const mpcx_traffic_actor *actors,
                                                    const double *actor_state, const double *tape, int64_t tape_rows,
                                                    const int32_t *actor_row, const mpcx_admit *admit, const mpcx_precedence *precedence) {
    if (mpcx_precedence_absent(precedence))
        return mpcx_admit_step_batch(ctx, ip, P, state, obs_off, obs_cnt, obs_skip, done, n_obs_pool, absent, n_actors, actors, actor_state, tape,
                                     tape_rows, actor_row, admit);
    if (!ctx) return MPCX_E_INVALID;
    // refused before the admission stage is launched: the scene of a stage call is its mask over the n_obs_pool rows
    const mpcx_scene scene = {absent, n_obs_pool, 0};
    int32_t rc = mpcx_precedence_validate(ctx, precedence, absent ? &scene : nullptr, admit);
    if (rc != MPCX_OK) return rc;
    rc = mpcx_admit_step_batch(ctx, ip, P, state, obs_off, obs_cnt, obs_skip, done, n_obs_pool, absent, n_actors, actors, actor_state, tape,
                               tape_rows, actor_row, admit);
    if (rc != MPCX_OK || P == 0 || precedence->mode != MPCX_PRECEDENCE_ENTRY) return rc;
    return mpcx_precedence_enqueue(ctx, P, obs_off, obs_skip, admit, precedence);
}
