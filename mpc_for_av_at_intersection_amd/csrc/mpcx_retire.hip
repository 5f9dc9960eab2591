// mpcx_retire.hip -- retirement at the goal in the device-resident closed loop: the reference's `if mpc.is_goal(state): break`
// (main/scenarios/mpc_intersection.py:92-93) per agent.  One lane per agent, one launch per step, LAST in the step (after record_kernel):
// evaluate the rule of mpcx_retire_core.h.  Everything it changes -- done, steps_driven, applied -- is device memory, so the launch has no
// step argument and a replayed hipGraph retires agents like a plain run.  The other kernels of the step read done[] through an optional
// pointer and leave a retired agent alone (mpcx_loop.hip has the list).  With a scene (mpcx_scene: departure) the arrival also sets the
// agent's word of the absent mask, which the next step's prediction, conflict search and record stage read.
#include "mpcx_common.h"
#include "mpcx_retire_core.h"
#include <cmath>

namespace mpcx {

__global__ __launch_bounds__(64) void retire_kernel(RetireArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    (void)retire_agent(a, q);
}

}  // namespace mpcx

// all-zero (or no) struct: "no retirement"
bool mpcx_retire_absent(const mpcx_retire *r) {
    return !r || (!r->done && !r->steps_driven && r->goal_dis == 0.0 && r->stop_speed == 0.0);
}

// the struct's own fields and what retirement needs of the run; never a GPU fault for a bad one
int32_t mpcx_retire_validate(mpcx_ctx *ctx, const mpcx_retire *r, int32_t P) {
    if (!r) return mpcx_fail(ctx, MPCX_E_INVALID, "retire: null struct");
    if (!r->done || !r->steps_driven)
        return mpcx_fail(ctx, MPCX_E_INVALID, "retire: done and steps_driven are both required (P zero-initialised int32 each), %s is null",
                         r->done ? "steps_driven" : "done");
    if (!std::isfinite(r->goal_dis) || !std::isfinite(r->stop_speed) || r->goal_dis < 0.0 || r->stop_speed < 0.0)
        return mpcx_fail(ctx, MPCX_E_INVALID, "retire: goal_dis and stop_speed must be finite and >= 0");
    if (P >= (1 << 24))
        return mpcx_fail(ctx, MPCX_E_INVALID, "retire: %d agents: no queue order is built from 2^24 agents on, and a retired agent is one that is not filed in it", P);
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "retire: %d linearisation passes: the later passes build their queue with the counting sort of "
                                              "mpcx_qp_solve_batch, which knows nothing of retired agents (not supported yet)", ctx->lin_passes);
    return MPCX_OK;
}

// all-zero (or no) struct: "no scene"
bool mpcx_scene_absent(const mpcx_scene *s) {
    return !s || (!s->absent && s->n_rows == 0 && s->reserved == 0);
}

// the scene against the run it is given with; never a GPU fault for a bad one.  The agents' own rows are read back (once per call, as the
// row maps of scripted traffic are): retire_kernel writes absent[obs_skip[q]]
int32_t mpcx_scene_validate(mpcx_ctx *ctx, const mpcx_scene *s, const mpcx_retire *retire, int32_t exchange, size_t pool_rows, const int32_t *obs_skip) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "scene: null struct");
    if (!retire) return mpcx_fail(ctx, MPCX_E_INVALID, "scene: departure needs retirement at the goal (mpcx_retire): it is the arrival that takes a car out");
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "scene: not supported in the agent-sharded layout (a remote rank's mask would have to travel with the all-gather)");
    if (!s->absent) return mpcx_fail(ctx, MPCX_E_INVALID, "scene: absent is null (n_rows zero-initialised int32)");
    if (s->n_rows < 0 || (size_t)s->n_rows != pool_rows)
        return mpcx_fail(ctx, MPCX_E_INVALID, "scene: n_rows = %d, the pool has %zu rows", s->n_rows, pool_rows);
    if (!obs_skip) return mpcx_fail(ctx, MPCX_E_INVALID, "scene: obs_skip is required (the agent's own pool row is the word its arrival sets)");
    return MPCX_OK;
}

// the launch alone (the struct has been checked): what the closed loop enqueues, also inside a capture
int32_t mpcx_retire_enqueue(mpcx_ctx *ctx, int32_t P, const double *state, double *applied, const double *path_xyyaw, const int32_t *path_off,
                            const int32_t *path_len, const int32_t *target_ind, const int32_t *goal_len, const mpcx_retire *r,
                            const mpcx_scene *scene, const int32_t *own_row) {
    mpcx::RetireArgs a{P, state, path_xyyaw, applied, path_off, path_len, target_ind, goal_len, *r};
    if (scene) { a.absent = scene->absent; a.own_row = own_row; a.n_rows = scene->n_rows; }
    hipLaunchKernelGGL(mpcx::retire_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "retire_kernel");
}
