// mpcx_route.hip -- routes in the device-resident closed loop: every vehicle of a respawning slot takes its own route from its own start
// pose, and the per-movement table of such a run is reduced on the device.  The rule is mpcx_route_core.h.
// respawn_route_kernel is launched IN PLACE OF respawn_kernel (mpcx_respawn.hip) when routes are given: one launch, one lane per agent, the
// last of a step.  A lane whose agent is driving leaves after loading done[q]; every access is to words of agent q plus the read-only route
// tables.  No LDS, no scratch.
// summary_kernel is one wavefront per instance striding over the instance's A G episode records, once per route; integer sums and a minimum
// through cross-lane shuffles: exact whatever the mapping, no floating-point atomics, no LDS.
#include "mpcx_common.h"
#include "mpcx_route_core.h"
#include <vector>

namespace mpcx {

__global__ __launch_bounds__(64) void respawn_route_kernel(RouteArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.r.P) return;
    if (a.r.done[q] == 0) return;           // driving
    (void)route_agent(a, q);
}

struct SummaryArgs {
    int A, G, R;
    const int32_t *served, *ep_i32;
    const double *ep_f64;
    long long *out_i64;
    double *out_f64;
};

__global__ __launch_bounds__(64) void summary_kernel(SummaryArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.A * a.G;                // records of the instance
    for (int r = 0; r < a.R; r++) {
        int64_t acc[4] = {0, 0, 0, 0};
        double lo = (double)INFINITY;
        for (int i = lane; i < n; i += WAVE) {
            const size_t q = (size_t)b * a.A + (size_t)(i / a.G);
            const int g = i % a.G;
            if (g >= a.served[q]) continue;
            const size_t e = q * (size_t)a.G + (size_t)g;
            const int32_t *w = a.ep_i32 + RESPAWN_I32 * e;
            if (w[7] != r) continue;
            summary_take(w, a.ep_f64 + RESPAWN_F64 * e, acc, lo);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] += (int64_t)__shfl_xor((long long)acc[k], s, WAVE);
            const double o = __shfl_xor(lo, s, WAVE);
            lo = o < lo ? o : lo;
        }
        if (lane == 0) {
            const size_t o = (size_t)b * a.R + (size_t)r;
#pragma unroll
            for (int k = 0; k < 4; k++) a.out_i64[4 * o + k] = (long long)acc[k];
            a.out_f64[o] = lo;
        }
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no routes"
bool mpcx_routes_absent(const mpcx_routes *s) {
    return !s || (s->n_routes == 0 && s->reserved == 0 && !s->route_off && !s->route_len && !s->route_of && !s->start_state && !s->start_idx &&
                  !s->path_off && !s->path_len);
}

// the struct's own fields and what routes need of the run; reads route_off / route_len back (R words each; never inside a capture).
// path_off / path_len: the descriptor's own, which the struct's must be.  max_len: the longest route the conflict search handles (0: not
// checked).  Never a GPU fault for a bad struct.
int32_t mpcx_routes_validate(mpcx_ctx *ctx, const mpcx_routes *s, const mpcx_respawn *respawn, const int32_t *path_off, const int32_t *path_len,
                             int32_t max_len) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "routes: null struct");
    if (!respawn)
        return mpcx_fail(ctx, MPCX_E_INVALID, "routes: routes need respawn (mpcx_respawn, and with it admission, a scene and retirement): a vehicle's route is written by the slot's reset");
    const char *missing = !s->route_off ? "route_off" : !s->route_len ? "route_len" : !s->route_of ? "route_of" : !s->start_state ? "start_state" :
                          !s->start_idx ? "start_idx" : !s->path_off ? "path_off" : !s->path_len ? "path_len" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "routes: route_off (R), route_len (R), route_of (P,G), start_state (P,G,4), start_idx (P,G), path_off (P) and path_len (P) are all required, %s is null", missing);
    if (s->n_routes < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "routes: n_routes = %d, at least one route", s->n_routes);
    if (s->path_off != path_off || s->path_len != path_len)
        return mpcx_fail(ctx, MPCX_E_INVALID, "routes: path_off and path_len must be the descriptor's own pointers (the stages read those words; the reset writes them)");
    std::vector<int32_t> len((size_t)s->n_routes), off((size_t)s->n_routes);
    if (hipMemcpy(len.data(), s->route_len, len.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(off.data(), s->route_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "routes: cannot read the route tables back for their check");
    for (int32_t r = 0; r < s->n_routes; r++) {
        if (len[r] < 1 || (max_len > 0 && len[r] > max_len))
            return mpcx_fail(ctx, MPCX_E_INVALID, "routes: route %d has %d points (1 .. %d, the interaction parameters' max_path_len)", r, len[r], max_len);
        if (off[r] < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "routes: route %d starts at path point %d", r, off[r]);
    }
    return MPCX_OK;
}

// the launch alone (the structs have been checked): what the closed loop enqueues in place of respawn_kernel, also inside a capture
int32_t mpcx_route_enqueue(mpcx_ctx *ctx, int32_t P, double *state, double *applied, double *u_sol, int32_t *traj_idx, int32_t *target_ind,
                           int32_t *cut_len, int32_t *iters, int32_t *prev_len, const int32_t *obs_skip, int32_t n_obs_pool,
                           const mpcx_run_log *log, const mpcx_retire *retire, const mpcx_admit *admit, const mpcx_respawn *respawn,
                           const mpcx_routes *routes) {
    mpcx::RouteArgs a = {};
    a.r.P = P; a.r.n_pool = n_obs_pool; a.r.u_len = 2 * ctx->mpc.T;
    a.r.has_log = log ? 1 : 0; a.r.has_prev_len = prev_len ? 1 : 0;
    a.r.state = state; a.r.applied = applied; a.r.u_sol = u_sol;
    a.r.traj_idx = traj_idx; a.r.target_ind = target_ind; a.r.cut_len = cut_len; a.r.iters = iters; a.r.prev_len = prev_len;
    a.r.own_row = obs_skip;
    a.r.done = retire->done; a.r.steps_driven = retire->steps_driven;
    a.r.ad = *admit;
    if (log) a.r.log = *log;
    a.r.rs = *respawn;
    a.rt = *routes;
    hipLaunchKernelGGL(mpcx::respawn_route_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "respawn_route_kernel");
}

extern "C" int32_t mpcx_respawn_step_batch_routes(mpcx_ctx *ctx, int32_t P, double *state, double *applied, double *u_sol, int32_t *traj_idx,
                                                  int32_t *target_ind, int32_t *cut_len, int32_t *iters, int32_t *prev_len,
                                                  const int32_t *obs_skip, int32_t n_obs_pool, const mpcx_run_log *log, const mpcx_retire *retire,
                                                  const mpcx_admit *admit, const mpcx_respawn *respawn, const mpcx_routes *routes,
                                                  int32_t max_path_len) {
    if (mpcx_routes_absent(routes))
        return mpcx_respawn_step_batch(ctx, P, state, applied, u_sol, traj_idx, target_ind, cut_len, iters, prev_len, obs_skip, n_obs_pool, log,
                                       retire, admit, respawn);
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (P < 0 || n_obs_pool < 0 || max_path_len < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "respawn_step_batch_routes: negative size");
    if (!respawn || mpcx_respawn_absent(respawn)) return mpcx_routes_validate(ctx, routes, nullptr, nullptr, nullptr, 0);
    if (P == 0) return MPCX_OK;             // nobody: nothing to check against, nothing to do
    if (!admit || !admit->wait || !admit->entered_step || !admit->clock)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: respawn needs admission (mpcx_admit with wait, entered_step and clock)");
    if (!retire || !retire->done || !retire->steps_driven)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn: respawn needs retirement (mpcx_retire with done and steps_driven)");
    int32_t rc = mpcx_respawn_validate(ctx, respawn, admit);
    if (rc != MPCX_OK) return rc;
    rc = mpcx_routes_validate(ctx, routes, respawn, routes->path_off, routes->path_len, max_path_len);
    if (rc != MPCX_OK) return rc;
    if (mpcx_record_absent(log)) log = nullptr;
    if (log) {
        rc = mpcx_record_validate(ctx, log, obs_skip);
        if (rc != MPCX_OK) return rc;
    }
    if (!state || !applied || !u_sol || !traj_idx || !target_ind || !cut_len || !iters || !obs_skip)
        return mpcx_fail(ctx, MPCX_E_INVALID, "respawn_step_batch_routes: null buffer (state, applied, u_sol, traj_idx, target_ind, cut_len, iters, obs_skip)");
    return mpcx_route_enqueue(ctx, P, state, applied, u_sol, traj_idx, target_ind, cut_len, iters, prev_len, obs_skip, n_obs_pool, log, retire, admit,
                              respawn, routes);
}

extern "C" int32_t mpcx_episode_summary(mpcx_ctx *ctx, int32_t P, int32_t A, int32_t G, int32_t R, const int32_t *served, const int32_t *ep_i32,
                                        const double *ep_f64, int64_t *out_i64, double *out_f64) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0 || G < 1 || R < 1 || (P > 0 && (A < 1 || P % A != 0)))
        return mpcx_fail(ctx, MPCX_E_INVALID, "episode_summary: P = %d slots in instances of A = %d, G = %d vehicles per slot, R = %d routes", P, A, G, R);
    if (P == 0) return MPCX_OK;
    if (!served || !ep_i32 || !ep_f64 || !out_i64 || !out_f64) return mpcx_fail(ctx, MPCX_E_INVALID, "episode_summary: null buffer");
    if ((long long)A * G > 0x7fffffffLL) return mpcx_fail(ctx, MPCX_E_INVALID, "episode_summary: A G = %lld records per instance", (long long)A * G);
    mpcx::SummaryArgs a{A, G, R, served, ep_i32, ep_f64, (long long *)out_i64, out_f64};
    hipLaunchKernelGGL(mpcx::summary_kernel, dim3(P / A), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "summary_kernel");
}
