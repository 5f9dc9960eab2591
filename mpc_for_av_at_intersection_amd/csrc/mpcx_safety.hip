// mpcx_safety.hip -- the near-miss log of the device-resident closed loop: the struct's checks, the setter that attaches it to the context,
// the stage and the conflict matrix.  The rule is mpcx_safety_core.h.
// safety_kernel: one launch directly behind the conflict search.  A LANE GROUP of SAFETY_G = 16 = MPCX_MAX_OBS lanes per agent, four agents
// per wavefront.  Lane j of the group owns slot j of the window: one sincos for its row's discs at the present pose, and its own walk over
// the frames of pred[r] (pred_steps x 32 contiguous bytes) against the agent's own frames, which are group-uniform loads; the walk stops at
// the first contact.  Then three group-wide minima: the distance, the slot that holds it, and the key frame << 8 | slot of the first
// contact (follow_min_key's shape).  The group's first lane runs the encounter rule and writes the agent's words.  A group whose agent is
// not measured leaves at once (group-uniform, and no shuffle crosses a group).  No LDS, no scratch, no atomics.
// safety_summary_kernel has summary_kernel's shape (mpcx_route.hip): one wavefront per instance striding over the instance's stored events,
// once per pair of classes; integer sums and minima through cross-lane shuffles, exact whatever the mapping.
#include "mpcx_common.h"
#include "mpcx_safety_core.h"
#include <cmath>
#include <cstring>

namespace mpcx {

constexpr int SAFETY_G = 16;
constexpr int SAFETY_WAVES = 4;
constexpr uint32_t SAFETY_NO_KEY = ~0u;
static_assert(SAFETY_G == MPCX_MAX_OBS, "one lane per slot of the window");

// the minimum of a 32-bit key over the lane group
__device__ __forceinline__ uint32_t safety_min_key(uint32_t key) {
#pragma unroll
    for (int m = SAFETY_G / 2; m >= 1; m >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)key, m, SAFETY_G);
        key = other < key ? other : key;
    }
    return key;
}

__global__ __launch_bounds__(64 * SAFETY_WAVES) void safety_kernel(SafetyArgs a) {
    const int sub = threadIdx.x & (SAFETY_G - 1);
    const int q = (int)((blockIdx.x * (unsigned)(64 * SAFETY_WAVES) + threadIdx.x) / SAFETY_G);
    if (q >= a.P) return;
    const int n = safety_slots(a, q);           // (group-uniform)
    if (n == 0) {
        if (sub == 0) safety_finish(a, q, safety_none());
        return;
    }
    const int32_t o = a.obs_skip[q];
    // ---- slot `sub`: one other row per lane, now and over the predicted frames
    const int32_t r = sub < n ? safety_slot_row(a, q, sub) : -1;
    double m = INFINITY;
    int32_t k = -1;
    if (r >= 0) {
        const double *e = a.obs6 + 6 * (size_t)o;
        double ed[4];
        rec_discs(a.cc, e[0], e[1], e[3], ed);
        const double now = safety_now(a, ed, r);
        if (now < m) m = now;                   // (a NaN stays out, as fmin keeps it out of the run log's minimum)
        k = safety_contact(a, o, r, safety_limit(a));
    }
    // ---- the nearest: the smallest distance, then the lowest slot that holds it
    double best = m;
#pragma unroll
    for (int x = SAFETY_G / 2; x >= 1; x >>= 1) {
        const double other = __shfl_xor(best, x, SAFETY_G);
        best = other < best ? other : best;
    }
    const uint32_t at = safety_min_key(m < (double)INFINITY && m == best ? (uint32_t)sub : SAFETY_NO_KEY);
    // ---- the first contact: the lowest frame, then the lowest slot
    const uint32_t key = safety_min_key(k >= 0 ? (uint32_t)k << 8 | (uint32_t)sub : SAFETY_NO_KEY);
    SafetyFound f = safety_none();
    const int32_t r_at = __shfl(r, at == SAFETY_NO_KEY ? 0 : (int)at, SAFETY_G);
    const int32_t r_key = __shfl(r, key == SAFETY_NO_KEY ? 0 : (int)(key & 255u), SAFETY_G);
    if (at != SAFETY_NO_KEY) { f.r_now = r_at; f.c_now = best - 2.0 * a.radius; }
    if (key != SAFETY_NO_KEY) { f.r_ttc = r_key; f.k_ttc = (int32_t)(key >> 8); }
    if (sub == 0) safety_finish(a, q, f);
}

struct SafetySummaryArgs {
    int A, capacity, R;
    double dt;
    const int32_t *route_off, *n_events, *ev_i32;
    const double *ev_f64;
    long long *out_i64;
    double *out_f64;
};

__global__ __launch_bounds__(64) void safety_summary_kernel(SafetySummaryArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.A * a.capacity;             // event slots of the instance
    const int C = a.R + 1;
    for (int ci = 0; ci < C; ci++)
        for (int cj = 0; cj < C; cj++) {
            int64_t acc[SAFETY_SUM_I64] = {0, 0, 0};
            double lo = (double)INFINITY;
            int32_t kmin = INT32_MAX;
            for (int i = lane; i < n; i += WAVE) {
                const size_t q = (size_t)b * a.A + (size_t)(i / a.capacity);
                const int e = i % a.capacity;
                if (e >= a.n_events[q]) continue;
                const size_t at = q * (size_t)a.capacity + (size_t)e;
                const int32_t *w = a.ev_i32 + SAFETY_I32 * at;
                if (safety_class(a.route_off, a.R, w[4]) != ci || safety_class(a.route_off, a.R, w[5]) != cj) continue;
                safety_take(w, a.ev_f64 + SAFETY_F64 * at, acc, lo, kmin);
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
                for (int k = 0; k < SAFETY_SUM_I64; k++) acc[k] += (int64_t)__shfl_xor((long long)acc[k], s, WAVE);
                const double ol = __shfl_xor(lo, s, WAVE);
                lo = ol < lo ? ol : lo;
                const int32_t ok = __shfl_xor(kmin, s, WAVE);
                kmin = ok < kmin ? ok : kmin;
            }
            if (lane == 0) {
                const size_t cell = ((size_t)b * C + (size_t)ci) * C + (size_t)cj;
#pragma unroll
                for (int k = 0; k < SAFETY_SUM_I64; k++) a.out_i64[SAFETY_SUM_I64 * cell + k] = (long long)acc[k];
                a.out_f64[SAFETY_SUM_F64 * cell] = lo;
                a.out_f64[SAFETY_SUM_F64 * cell + 1] = safety_seconds(kmin, a.dt);
            }
        }
}

}  // namespace mpcx

// all-zero (or no) struct: "no safety stage"
bool mpcx_safety_absent(const mpcx_safety *s) {
    return !s || (!s->partner && !s->clearance && !s->ttc_row && !s->ttc_frame && !s->tick && !s->enc_row && !s->n_events && !s->ev_i32 &&
                  !s->ev_f64 && !s->row_agent && s->near == 0.0 && s->ttc_frames == 0 && s->capacity == 0 && s->n_rows == 0 && s->n_pool == 0 &&
                  s->reserved == 0);
}

// the struct's own fields and what the stage needs of the run.  n_pool: the run's pool rows; exchange: the descriptor's (0 for a stage
// call).  Never a GPU fault for a bad struct.
int32_t mpcx_safety_validate(mpcx_ctx *ctx, const mpcx_safety *s, const mpcx_interaction_params *ip, int32_t P, int32_t n_pool, int32_t exchange) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: null struct");
    if (!ip) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: null interaction parameters");
    const char *missing = !s->partner ? "partner" : !s->clearance ? "clearance" : !s->ttc_row ? "ttc_row" : !s->ttc_frame ? "ttc_frame"
                        : !s->tick ? "tick" : !s->enc_row ? "enc_row" : !s->n_events ? "n_events" : !s->row_agent ? "row_agent" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety: %s is null (partner, clearance, ttc_row, ttc_frame, tick, enc_row, n_events: n_rows words each; row_agent: n_pool)", missing);
    if (s->capacity < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: capacity = %d is negative", s->capacity);
    if (s->capacity > 0 && (!s->ev_i32 || !s->ev_f64))
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety: ev_i32 or ev_f64 is null with capacity = %d (n_rows x capacity x 8 int32, x 2 doubles)", s->capacity);
    if (s->n_rows != P) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: n_rows = %d is not P = %d", s->n_rows, P);
    if (s->n_pool != n_pool) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: n_pool = %d is not the run's %d pool rows", s->n_pool, n_pool);
    if (!std::isfinite(s->near) || s->near < 0.0) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: near = %g must be finite and not negative", s->near);
    if (ip->pred_steps < 1 || ip->pred_steps > MPCX_PRED_STEPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety: pred_steps outside 1..%d", MPCX_PRED_STEPS_MAX);
    if (s->ttc_frames < 0 || s->ttc_frames > ip->pred_steps)
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety: ttc_frames = %d outside 0..pred_steps = %d", s->ttc_frames, ip->pred_steps);
    if (!std::isfinite(ip->radius) || ip->radius < 0.0) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: radius = %g must be finite and not negative", ip->radius);
    if (s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: the reserved word is not 0");
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety: not supported in the agent-sharded layout (shard by instances)");
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_safety(mpcx_ctx *ctx, const mpcx_safety *s) {
    if (!ctx) return MPCX_E_INVALID;
    memset(&ctx->safety, 0, sizeof ctx->safety);                // (padding too: the cached graph's key takes the struct as it stands)
    ctx->have_safety = !mpcx_safety_absent(s);
    if (ctx->have_safety) {
        mpcx_safety &f = ctx->safety;
        f.partner = s->partner; f.clearance = s->clearance; f.ttc_row = s->ttc_row; f.ttc_frame = s->ttc_frame; f.tick = s->tick;
        f.enc_row = s->enc_row; f.n_events = s->n_events; f.ev_i32 = s->ev_i32; f.ev_f64 = s->ev_f64; f.row_agent = s->row_agent;
        f.near = s->near; f.ttc_frames = s->ttc_frames; f.capacity = s->capacity; f.n_rows = s->n_rows; f.n_pool = s->n_pool;
        f.reserved = s->reserved;
    }
    return MPCX_OK;
}

// the launch alone (the struct has been checked; pred holds n_obs_pool x pred_steps frames): what the closed loop enqueues, also inside a
// capture
int32_t mpcx_safety_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *path_off,
                            const int32_t *traj_idx, const int32_t *done, int32_t n_obs_pool, const double *obs6, const double *pred,
                            const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip, const int32_t *absent,
                            const mpcx_safety *safety) {
    mpcx::SafetyArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.n_pool = n_obs_pool; a.pred_steps = ip->pred_steps; a.radius = ip->radius;
    for (int i = 0; i < 4; i++) a.cc[i] = ip->circle_centers[i];
    a.obs6 = obs6; a.pred = pred; a.state = state; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip; a.traj_idx = traj_idx;
    a.path_off = path_off; a.done = done; a.absent = absent;
    a.s = *safety;
    const int per_block = 64 * mpcx::SAFETY_WAVES / mpcx::SAFETY_G;
    hipLaunchKernelGGL(mpcx::safety_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::SAFETY_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "safety_kernel");
}

extern "C" int32_t mpcx_safety_step_batch(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state,
                                          const int32_t *path_off, const int32_t *traj_idx, const int32_t *done, int32_t n_obs_pool,
                                          const double *obs6, const double *pred, const int32_t *obs_off, const int32_t *obs_cnt,
                                          const int32_t *obs_skip, const int32_t *absent, const mpcx_safety *safety) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0 || n_obs_pool < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "safety_step_batch: negative size");
    const int32_t rc = mpcx_safety_validate(ctx, safety, ip, P, n_obs_pool, 0);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !traj_idx || !obs_off || !obs_cnt || !obs_skip || (n_obs_pool > 0 && !obs6))
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety_step_batch: null buffer (state, path_off, traj_idx, obs6, obs_off, obs_cnt, obs_skip)");
    if (!pred) {            // the context's own prediction, as its last conflict search left it
        if (n_obs_pool > 0 && (!ctx->pred || ctx->pred_cap < (size_t)n_obs_pool * ip->pred_steps * 4 * sizeof(double)))
            return mpcx_fail(ctx, MPCX_E_INVALID, "safety_step_batch: pred is null and the context holds no prediction of %d rows x %d frames", n_obs_pool, ip->pred_steps);
        pred = ctx->pred;
    }
    return mpcx_safety_enqueue(ctx, ip, P, state, path_off, traj_idx, done, n_obs_pool, obs6, pred, obs_off, obs_cnt, obs_skip, absent, safety);
}

extern "C" int32_t mpcx_safety_summary(mpcx_ctx *ctx, int32_t P, int32_t A, int32_t capacity, int32_t R, const int32_t *route_off, double dt,
                                       const int32_t *n_events, const int32_t *ev_i32, const double *ev_f64, int64_t *out_i64,
                                       double *out_f64) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0 || A < 1 || P % A != 0 || capacity < 0 || R < 0 || !(dt > 0) || !std::isfinite(dt))
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety_summary: P = %d agents in instances of A = %d, capacity = %d, R = %d routes, dt = %g", P, A, capacity, R, dt);
    if (P == 0) return MPCX_OK;
    if (!n_events || !out_i64 || !out_f64 || (R > 0 && !route_off) || (capacity > 0 && (!ev_i32 || !ev_f64)))
        return mpcx_fail(ctx, MPCX_E_INVALID, "safety_summary: null buffer");
    if ((long long)A * capacity > 0x7fffffffLL) return mpcx_fail(ctx, MPCX_E_INVALID, "safety_summary: A capacity = %lld event slots per instance", (long long)A * capacity);
    mpcx::SafetySummaryArgs a{A, capacity, R, dt, route_off, n_events, ev_i32, ev_f64, (long long *)out_i64, out_f64};
    hipLaunchKernelGGL(mpcx::safety_summary_kernel, dim3(P / A), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "safety_summary_kernel");
}
