// mpcx_traffic.hip -- scripted traffic on the device: the cars of the reference's scenarios that follow a hard-wired steering rule
// and never yield (main/lib/moving_obstacles.py:16-231; stepped by scenarios/mpc_intersection.py:118-122,155-156).  One lane per
// actor: write the actor's get() row into its row of the obstacle pool, then advance its state (mpcx_traffic_core.h).  All mutable
// state is device memory, so the launch has no step argument and a replayed hipGraph keeps advancing the actors.
#include "mpcx_common.h"
#include "mpcx_traffic_core.h"
#include <vector>

namespace mpcx {

struct TrafficArgs {
    int n, n_pool;
    const mpcx_traffic_actor *actors;
    double *state;          // [n][4]: x, y, theta, counter / cursor
    const double *tape;     // [tape_rows][6]
    int64_t tape_rows;
    const int32_t *pool_row;
    double *obs6;
};

__global__ __launch_bounds__(64) void traffic_kernel(TrafficArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const mpcx_traffic_actor act = a.actors[i];
    double st[4], row[6];
    double *sp = a.state + 4 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 4; k++) st[k] = sp[k];
    traffic_get_step(act, st, a.tape, a.tape_rows, row);
    const int r = a.pool_row[i];
    if (r >= 0 && r < a.n_pool) {           // (the host has checked the table; a row outside the pool is never written)
        double *o = a.obs6 + 6 * (size_t)r;
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = row[k];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) sp[k] = st[k];
}

}  // namespace mpcx

// The actor table and the row map live in device memory: they are read back and checked -- kinds, TAPE actors inside the uploaded
// table, rows inside the pool -- once per call of an entry point (mpcx_traffic_step_batch; mpcx_closed_loop_run: once per run of
// n_steps, before the first launch and outside any stream capture), which synchronises the stream.  The kernel clamps all the same.
int32_t mpcx_traffic_validate(mpcx_ctx *ctx, int32_t n_actors, const mpcx_traffic_actor *actors, const double *tape, int64_t tape_rows,
                              const int32_t *pool_row, int32_t n_obs_pool) {
    std::vector<mpcx_traffic_actor> act((size_t)n_actors);
    std::vector<int32_t> rows((size_t)n_actors);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(act.data(), actors, act.size() * sizeof(mpcx_traffic_actor), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rows.data(), pool_row, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "traffic: cannot read the actor table back for its check");
    for (int i = 0; i < n_actors; i++) {
        const mpcx_traffic_actor &a = act[i];
        if (a.kind < MPCX_TRAFFIC_TINTERSECTION || a.kind > MPCX_TRAFFIC_TAPE)
            return mpcx_fail(ctx, MPCX_E_INVALID, "traffic: actor %d has kind %d", i, a.kind);
        if (rows[i] < 0 || rows[i] >= n_obs_pool)
            return mpcx_fail(ctx, MPCX_E_INVALID, "traffic: actor %d writes pool row %d of %d", i, rows[i], n_obs_pool);
        if (a.kind == MPCX_TRAFFIC_TAPE) {
            if (!tape || tape_rows <= 0) return mpcx_fail(ctx, MPCX_E_INVALID, "traffic: actor %d is a TAPE actor and no table was given", i);
            const int64_t last = (int64_t)a.tape_off + (int64_t)(a.tape_rows - 1) * a.tape_stride;
            if (a.tape_rows < 1 || a.tape_off < 0 || a.tape_stride < 0 || last >= tape_rows)
                return mpcx_fail(ctx, MPCX_E_INVALID, "traffic: the tape of actor %d (first row %d, %d rows, stride %d) leaves the table of %lld rows",
                                 i, a.tape_off, a.tape_rows, a.tape_stride, (long long)tape_rows);
        } else if (!(a.L > 0) || !(a.model_dt > 0) || !(a.counter_dt > 0) || (a.direction != 1 && a.direction != -1)) {
            return mpcx_fail(ctx, MPCX_E_INVALID, "traffic: actor %d needs L, model_dt, counter_dt > 0 and direction +-1", i);
        }
    }
    return MPCX_OK;
}

// the launch alone (the table has been checked): what mpcx_closed_loop_run enqueues, also inside a capture
int32_t mpcx_traffic_enqueue(mpcx_ctx *ctx, int32_t n_actors, const mpcx_traffic_actor *actors, double *actor_state, const double *tape,
                             int64_t tape_rows, const int32_t *pool_row, int32_t n_obs_pool, double *obs6) {
    mpcx::TrafficArgs ta{n_actors, n_obs_pool, actors, actor_state, tape, tape ? tape_rows : (int64_t)0, pool_row, obs6};
    hipLaunchKernelGGL(mpcx::traffic_kernel, dim3((n_actors + 63) / 64), dim3(64), 0, ctx->stream, ta);
    return mpcx_check_launch(ctx, "traffic_kernel");
}

extern "C" int32_t mpcx_traffic_step_batch(mpcx_ctx *ctx, int32_t n_actors, const mpcx_traffic_actor *actors, double *actor_state,
                                           const double *tape, int64_t tape_rows, const int32_t *pool_row, int32_t n_obs_pool,
                                           double *obs6) {
    if (!ctx) return MPCX_E_INVALID;
    if (n_actors == 0) return MPCX_OK;
    if (n_actors < 0 || n_obs_pool < 0 || tape_rows < 0 || !actors || !actor_state || !pool_row || !obs6)
        return mpcx_fail(ctx, MPCX_E_INVALID, "traffic_step_batch: null pointer or negative size");
    int32_t rc = mpcx_traffic_validate(ctx, n_actors, actors, tape, tape_rows, pool_row, n_obs_pool);
    if (rc != MPCX_OK) return rc;
    return mpcx_traffic_enqueue(ctx, n_actors, actors, actor_state, tape, tape_rows, pool_row, n_obs_pool, obs6);
}
