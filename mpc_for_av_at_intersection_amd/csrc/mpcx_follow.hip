// mpcx_follow.hip -- car following in the device-resident closed loop: the struct's checks, the setter that attaches it to the context and
// the two stages.  The rule is mpcx_follow_core.h.
// follow_kernel: one launch behind the signal / actuated / reserve stage (behind the conflict search where there are no signals), in both
// stop modes.  A LANE GROUP of FOLLOW_G = 16 = MPCX_MAX_OBS lanes per agent, four agents per wavefront.  Lane j of the group loads the
// window's slot j (x, y, v, yaw of one other row) once; sixteen shuffles hand every lane the (x, y) of every slot.  The lanes then stride
// over the scanned path points, each point loaded once by one lane, and keep a running (d^2, k) per slot in registers.  The per-slot
// argmin over the group is a REDUCE-SCATTER butterfly: in the round with mask m a lane sends its partner (__shfl_xor) the m slots the
// partner keeps and folds the m it receives into its own, (d^2, k) compared as one key, d^2 first -- 8 + 4 + 2 + 1 exchanges instead of
// 16 x 4, and lane j ends with the projection of slot j, the row it loaded itself: the candidate test needs nothing from another lane.  The
// final choice is a group-wide minimum of k* << 8 | slot, as reserve_kernel orders its grants; the group's first lane does the stop point
// and the cap and writes the agent's words.  A group whose agent is retired or has no window leaves at once (group-uniform, and no
// shuffle crosses a group).  No LDS, no scratch, no atomics.
// follow_clamp_kernel has the shape of advise_kernel's clamp part: lane i of a wavefront reads the cap of agent b0 + i, then floor(64 /
// (T + 1)) agents per pass, each on a run of T + 1 lanes of its own; a wavefront or a pass without a capped agent is skipped, both
// conditions wave-uniform.  Everything either kernel reads is device memory, so a replayed hipGraph behaves like a plain run.
#include "mpcx_common.h"
#include "mpcx_follow_core.h"
#include <cmath>
#include <cstring>

namespace mpcx {

constexpr int FOLLOW_G = 16;
constexpr int FOLLOW_WAVES = 4;
constexpr uint64_t FOLLOW_NO_KEY = ~0ull;
static_assert(FOLLOW_G == MPCX_MAX_OBS, "one lane per slot of the window");

// one round of the reduce-scatter: the N slots D[0 .. N) become N / 2; a lane whose bit N / 2 is set keeps the upper half
template <int N>
__device__ __forceinline__ void follow_fold(double (&D)[FOLLOW_G], int32_t (&K)[FOLLOW_G], int sub) {
    const bool up = (sub & (N / 2)) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
        const double send_d = up ? D[i] : D[i + N / 2], keep_d = up ? D[i + N / 2] : D[i];
        const int32_t send_k = up ? K[i] : K[i + N / 2], keep_k = up ? K[i + N / 2] : K[i];
        const double od = __shfl_xor(send_d, N / 2, FOLLOW_G);
        const int32_t ok = __shfl_xor(send_k, N / 2, FOLLOW_G);
        const bool take = od < keep_d || (od == keep_d && ok < keep_k);       // the lowest k of equal distances
        D[i] = take ? od : keep_d;
        K[i] = take ? ok : keep_k;
    }
}

// the minimum of a 64-bit key over the lane group
__device__ __forceinline__ uint64_t follow_min_key(uint64_t key) {
#pragma unroll
    for (int m = FOLLOW_G / 2; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, m, FOLLOW_G), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), m, FOLLOW_G);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        key = other < key ? other : key;
    }
    return key;
}

__global__ __launch_bounds__(64 * FOLLOW_WAVES) void follow_kernel(FollowArgs a) {
    const int sub = threadIdx.x & (FOLLOW_G - 1);
    const int q = (int)((blockIdx.x * (unsigned)(64 * FOLLOW_WAVES) + threadIdx.x) / FOLLOW_G);
    if (q >= a.P) return;
    const int n = follow_slots(a, q);           // (group-uniform)
    if (n == 0) {
        if (sub == 0) follow_finish(a, q, FollowLeader{-1, 0, 0.0});
        return;
    }
    const int32_t ti = a.traj_idx[q], last = follow_last(a, q);
    const double *path = a.path_xyyaw + 3 * (size_t)a.path_off[q];
    // ---- slot `sub`: one other row per lane
    const int32_t r = sub < n ? follow_slot_row(a, q, sub) : -1;
    double ox = 0.0, oy = 0.0, ov = 0.0, oyaw = 0.0;
    if (r >= 0) {
        const double *o = a.obs6 + 6 * (size_t)r;
        ox = o[0]; oy = o[1]; ov = o[2]; oyaw = o[3];
    }
    double X[FOLLOW_G], Y[FOLLOW_G], D[FOLLOW_G];
    int32_t K[FOLLOW_G];
#pragma unroll
    for (int j = 0; j < FOLLOW_G; j++) {
        X[j] = __shfl(ox, j, FOLLOW_G);
        Y[j] = __shfl(oy, j, FOLLOW_G);
        D[j] = INFINITY;
        K[j] = INT32_MAX;
    }
    // ---- the scan: the group's lanes stride over the points, ascending, so `<` keeps a lane's lowest k.  A slot beyond the group's n is
    // nobody's candidate and is not measured: group-uniform, so the wavefront skips it where its four windows agree (they mostly do)
    for (int32_t k = ti + sub; k <= last; k += FOLLOW_G) {
        const double px = path[3 * (size_t)k], py = path[3 * (size_t)k + 1];
#pragma unroll
        for (int j = 0; j < FOLLOW_G; j++) {
            if (j < n) {
                const double d = follow_d2(px, py, X[j], Y[j]);
                if (d < D[j]) { D[j] = d; K[j] = k; }
            }
        }
    }
    // ---- the per-slot argmin over the group: lane `sub` ends with slot `sub` in D[0], K[0]
    follow_fold<16>(D, K, sub);
    follow_fold<8>(D, K, sub);
    follow_fold<4>(D, K, sub);
    follow_fold<2>(D, K, sub);
    const int32_t ks = K[0];
    const bool cand = r >= 0 && ks <= last && follow_candidate(a, ti, D[0], ks, path[3 * (size_t)ks + 2], oyaw);
    // ---- the leader: the smallest k*, then the lowest slot
    const uint64_t key = follow_min_key(cand ? (uint64_t)(uint32_t)ks << 8 | (uint64_t)sub : FOLLOW_NO_KEY);
    const int from = key == FOLLOW_NO_KEY ? 0 : (int)(key & 255u);
    FollowLeader ld{__shfl(r, from, FOLLOW_G), (int32_t)(key >> 8), __shfl(ov, from, FOLLOW_G)};
    if (key == FOLLOW_NO_KEY) ld.row = -1;
    if (sub == 0) follow_finish(a, q, ld);
}

constexpr int FOLLOW_CLAMP_AGENTS = 16;

__global__ __launch_bounds__(64 * FOLLOW_WAVES) void follow_clamp_kernel(FollowArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = a.W;
    const int b0 = ((int)blockIdx.x * FOLLOW_WAVES + wave) * FOLLOW_CLAMP_AGENTS;
    const int nag = a.P - b0 < FOLLOW_CLAMP_AGENTS ? a.P - b0 : FOLLOW_CLAMP_AGENTS;      // agents of this wavefront (<= 0: none)
    if (nag <= 0) return;
    double v = 0.0;
    if (lane < nag && !(a.done && a.done[b0 + lane] != 0)) v = a.fl.cap[b0 + lane];
    if (__ballot(v > 0.0) == 0) return;
    // ---- the clamp: lane = (agent g of the pass, window point t)
    const int G = 64 / W;
    const int g = lane / W, t = lane - g * W;
    for (int base = 0; base < nag; base += G) {
        const int i = base + g;
        const bool on = g < G && i < nag;
        const double vi = __shfl(v, on ? i : 0);
        const bool cap = on && vi > 0.0;
        if (__ballot(cap) == 0) continue;
        if (cap) follow_clamp(a, b0 + i, t, vi);
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no following"
bool mpcx_following_absent(const mpcx_following *s) {
    return !s || (!s->leader && !s->gap && !s->cap && s->standstill == 0.0 && s->time_gap == 0.0 && s->brake == 0.0 && s->v_min == 0.0 &&
                  s->lateral == 0.0 && s->heading == 0.0 && s->reach == 0 && s->n_rows == 0 && s->reserved == 0);
}

// the struct's own fields and what following needs of the run.  exchange: the descriptor's (0 for a stage call).  Never a GPU fault for a
// bad struct.
int32_t mpcx_following_validate(mpcx_ctx *ctx, const mpcx_following *s, int32_t P, int32_t exchange) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "following: null struct");
    const char *missing = !s->leader ? "leader" : !s->gap ? "gap" : !s->cap ? "cap" : nullptr;
    if (missing) return mpcx_fail(ctx, MPCX_E_INVALID, "following: %s is null (leader, gap and cap: n_rows words each, one per agent)", missing);
    if (s->n_rows != P) return mpcx_fail(ctx, MPCX_E_INVALID, "following: n_rows = %d is not P = %d", s->n_rows, P);
    const struct { const char *name; double v; } pos[4] = {{"standstill", s->standstill}, {"brake", s->brake}, {"lateral", s->lateral}, {"heading", s->heading}};
    for (const auto &f : pos)
        if (!std::isfinite(f.v) || !(f.v > 0.0)) return mpcx_fail(ctx, MPCX_E_INVALID, "following: %s = %g must be finite and positive", f.name, f.v);
    if (!std::isfinite(s->time_gap) || s->time_gap < 0.0)
        return mpcx_fail(ctx, MPCX_E_INVALID, "following: time_gap = %g must be finite and not negative", s->time_gap);
    if (!std::isfinite(s->v_min) || !(s->v_min > 0.0)) return mpcx_fail(ctx, MPCX_E_INVALID, "following: v_min = %g must be finite and positive", s->v_min);
    if (s->reach < 1 || s->reach > MPCX_MAX_REMAINING)
        return mpcx_fail(ctx, MPCX_E_INVALID, "following: reach = %d outside 1..%d path points", s->reach, MPCX_MAX_REMAINING);
    if (s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "following: the reserved word is not 0");
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "following: not supported in the agent-sharded layout (shard by instances)");
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_following(mpcx_ctx *ctx, const mpcx_following *s) {
    if (!ctx) return MPCX_E_INVALID;
    memset(&ctx->following, 0, sizeof ctx->following);          // (padding too: the cached graph's key takes the struct as it stands)
    ctx->have_following = !mpcx_following_absent(s);
    if (ctx->have_following) {
        mpcx_following &f = ctx->following;
        f.leader = s->leader; f.gap = s->gap; f.cap = s->cap;
        f.standstill = s->standstill; f.time_gap = s->time_gap; f.brake = s->brake; f.v_min = s->v_min; f.lateral = s->lateral;
        f.heading = s->heading; f.reach = s->reach; f.n_rows = s->n_rows; f.reserved = s->reserved;
    }
    return MPCX_OK;
}

static mpcx::FollowArgs follow_args(int32_t P, int32_t W, int32_t n_pool, bool speed, double dl, const mpcx_following *following) {
    mpcx::FollowArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.W = W; a.n_pool = n_pool; a.speed = speed ? 1 : 0; a.dl = dl;
    a.fl = *following;
    return a;
}

// the launches alone (the struct has been checked): what the closed loop enqueues, also inside a capture
int32_t mpcx_follow_enqueue(mpcx_ctx *ctx, int32_t P, double dl, bool speed, const double *state, const double *path_xyyaw,
                            const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                            int32_t n_obs_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip,
                            const int32_t *absent, const mpcx_following *following) {
    mpcx::FollowArgs a = follow_args(P, 0, n_obs_pool, speed, dl, following);
    a.state = state; a.path_xyyaw = path_xyyaw; a.path_off = path_off; a.path_len = path_len; a.traj_idx = traj_idx; a.cut_len = cut_len;
    a.done = done; a.obs6 = obs6; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip; a.absent = absent;
    const int per_block = 64 * mpcx::FOLLOW_WAVES / mpcx::FOLLOW_G;
    hipLaunchKernelGGL(mpcx::follow_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::FOLLOW_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "follow_kernel");
}

int32_t mpcx_follow_cap_enqueue(mpcx_ctx *ctx, int32_t P, const int32_t *done, const mpcx_following *following, double *xref) {
    mpcx::FollowArgs a = follow_args(P, ctx->mpc.T + 1, 0, true, 0.0, following);
    a.done = done; a.xref = xref;
    const int per_block = mpcx::FOLLOW_WAVES * mpcx::FOLLOW_CLAMP_AGENTS;
    hipLaunchKernelGGL(mpcx::follow_clamp_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::FOLLOW_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "follow_clamp_kernel");
}

extern "C" int32_t mpcx_follow_step_batch(mpcx_ctx *ctx, int32_t P, double dl, int32_t stop_mode, const double *state, const double *path_xyyaw,
                                          const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len,
                                          const int32_t *done, int32_t n_obs_pool, const double *obs6, const int32_t *obs_off,
                                          const int32_t *obs_cnt, const int32_t *obs_skip, const int32_t *absent, const mpcx_following *following) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0 || n_obs_pool < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "follow_step_batch: negative size");
    if (stop_mode != MPCX_STOP_CUT && stop_mode != MPCX_STOP_SPEED)
        return mpcx_fail(ctx, MPCX_E_INVALID, "follow_step_batch: unknown stop mode %d (MPCX_STOP_CUT or MPCX_STOP_SPEED)", stop_mode);
    const int32_t rc = mpcx_following_validate(ctx, following, P, 0);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_xyyaw || !path_off || !path_len || !traj_idx || !cut_len || !obs6 || !obs_off || !obs_cnt || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "follow_step_batch: null buffer (state, path_xyyaw, path_off, path_len, traj_idx, cut_len, obs6, obs_off, obs_cnt) or dl <= 0");
    return mpcx_follow_enqueue(ctx, P, dl, stop_mode == MPCX_STOP_SPEED, state, path_xyyaw, path_off, path_len, traj_idx, cut_len, done, n_obs_pool,
                               obs6, obs_off, obs_cnt, obs_skip, absent, following);
}

extern "C" int32_t mpcx_follow_cap_step_batch(mpcx_ctx *ctx, int32_t P, const int32_t *done, const mpcx_following *following, double *xref) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "follow_cap_step_batch: negative size");
    const int32_t rc = mpcx_following_validate(ctx, following, P, 0);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!xref) return mpcx_fail(ctx, MPCX_E_INVALID, "follow_cap_step_batch: xref is null");
    return mpcx_follow_cap_enqueue(ctx, P, done, following, xref);
}
