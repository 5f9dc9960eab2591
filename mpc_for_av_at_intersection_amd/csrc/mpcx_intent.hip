// mpcx_intent.hip -- shared plans in the device-resident closed loop: the struct's checks and the stage that re-rolls the last MPC solution
// of a sharing agent into its own pool row's predicted frames.  The rule is mpcx_intent_core.h.
// intent_kernel: one launch between the prediction and the conflict search.  A wavefront takes INT_AGENTS consecutive agents, each on a
// group of INT_GROUP lanes of its own (a block is INT_WAVES wavefronts).  Lane 0 of a group writes frames[q]; a wavefront with no sharing,
// driving agent leaves after that store (wave-uniform ballot, as advise_kernel).  The frames of an agent go INT_GROUP at a time, frame
// base + i on lane i of its group:
//   * the planned controls of the pass are INT_GROUP consecutive doubles of each row of the agent's u_sol (one coalesced load per row),
//     and the tangent of a planned steering angle is taken on the lane of the frame that uses it.  Once every frame of a pass lies beyond
//     the plan (wave-uniform: T is the launch's) the last column, taken once before the loop, serves and no load or tangent is issued.
//   * speed and heading are sums over the frames: v adds acc dt, yaw adds ((v / L) tan steer) dt, and neither needs a sine.  Each is a
//     group_chain (mpcx_common.h): every lane walks the INT_GROUP additions in frame order on terms handed over by shuffle -- the operations
//     of one lane walking the frames alone, on the same operands -- and keeps the value of its own frame.
//   * so the sincos of the INT_GROUP headings of a pass are independent: one per lane, side by side.  predict_kernel, one lane per row,
//     takes pred_steps of them one after the other; here a wavefront issues ceil(pred_steps / INT_GROUP).
//   * x and y are again chains, on v cos yaw and v sin yaw of the pose BEFORE the frame (the neighbour lane's, group_prev); the two disc
//     centres (pose_discs) and the 32-byte store of a frame are its lane's: a group writes INT_GROUP consecutive frames, coalesced.
// The carry into the next pass (x, y, v, yaw, cos, sin after the pass's last frame) is the same in every lane of the group.
// A group whose agent does not share runs along masked: it loads nothing and stores nothing.  Every access is to words of the wavefront's
// own agents: state, u_sol, status, share, done, obs_skip of agent q, absent and the frames of row obs_skip[q] (checked against the pool
// here too), frames[q].  No LDS, no scratch, no atomics.  Everything it reads is device memory, so a replayed hipGraph behaves like a plain
// run.
#include "mpcx_common.h"
#include "mpcx_intent_core.h"
#include <cstring>
#include <vector>

namespace mpcx {

constexpr int INT_WAVES = 4;
constexpr int INT_GROUP = 4;
constexpr int INT_AGENTS = WAVE / INT_GROUP;
static_assert(INT_GROUP >= 2 && (INT_GROUP & (INT_GROUP - 1)) == 0 && INT_GROUP <= WAVE, "a lane group is a power of two (group_chain)");

__global__ __launch_bounds__(64 * INT_WAVES) void intent_kernel(IntentArgs a) {
    constexpr int G = INT_GROUP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & (G - 1);
    const int q = ((int)blockIdx.x * INT_WAVES + wave) * INT_AGENTS + lane / G;
    const int S = a.ip.pred_steps, T = a.T;
    int32_t r = -1;
    if (q < a.P) {
        r = intent_row(a, q);
        if (i == 0) a.in.frames[q] = r < 0 ? 0 : S;
    }
    const bool on = r >= 0;
    if (__ballot(on) == 0) return;
    const double dt = a.ip.dt, L = a.ip.L;
    const double *u = a.u_sol + 2 * (size_t)T * (size_t)(on ? q : 0);
    double *out = a.pred + (size_t)(on ? r : 0) * (size_t)S * 4;
    // ---- the pose the plan starts from, and the plan's last column (what every frame beyond the plan takes)
    double X = 0.0, Y = 0.0, V = 0.0, YAW = 0.0, adt_last = 0.0, tn_last = 0.0;
    if (on) {
        const double *st = a.state + 4 * (size_t)q;
        X = st[0]; Y = st[1]; V = st[2]; YAW = st[3];
        adt_last = intent_impulse(u[T - 1], dt);
        tn_last = tan(u[2 * T - 1]);
    }
    double Sn, Cs;
    sincos(YAW, &Sn, &Cs);
    const auto add = [](double sum, double term) { return intent_speed(sum, term); };
    const auto step = [dt](double sum, double term) { return intent_step(sum, term, dt); };
    for (int base = 0; base < S; base += G) {
        const int k = base + i;
        // ---- the controls of frame k (wave-uniform branch: base and T are the launch's)
        double adt = adt_last, tn = tn_last;
        if (base + 1 < T - 1 && on) {
            const int j = intent_col(T, k);
            adt = intent_impulse(u[j], dt);
            tn = tan(u[T + j]);
        }
        // ---- speed and heading after frame k
        const double v_in = V;
        const double v = group_chain<G>(V, adt, i, add);
        const double yaw = group_chain<G>(YAW, intent_turn(v, L, tn), i, step);
        double s, c;
        sincos(yaw, &s, &c);
        // ---- position: the terms are those of the pose before the frame
        const double vp = group_prev<G>(v, v_in, i), cp = group_prev<G>(c, Cs, i), sp = group_prev<G>(s, Sn, i);
        const double x = group_chain<G>(X, intent_along(vp, cp), i, step);
        const double y = group_chain<G>(Y, intent_along(vp, sp), i, step);
        if (on && k < S) pose_discs(a.ip, x, y, c, s, out + 4 * (size_t)k);
        Cs = __shfl(c, G - 1, G);
        Sn = __shfl(s, G - 1, G);
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no sharing"
bool mpcx_intent_absent(const mpcx_intent *s) { return !s || (!s->share && !s->frames && s->n_rows == 0 && s->reserved == 0); }

// the struct's own fields and what the stage needs of the run: the local pool, and every agent's own row inside it (read back once, as
// mpcx_loop_check_rows does for the scripted traffic's rows).  Never a GPU fault for a bad struct.
int32_t mpcx_intent_validate(mpcx_ctx *ctx, const mpcx_intent *s, int32_t P, int32_t exchange, int32_t pool_rows, const int32_t *obs_skip) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "intent: null struct");
    if (!s->share) return mpcx_fail(ctx, MPCX_E_INVALID, "intent: share is null (n_rows int32, one per agent: nonzero = the agent shares its plan)");
    if (!s->frames) return mpcx_fail(ctx, MPCX_E_INVALID, "intent: frames is null (n_rows int32, one per agent, out)");
    if (s->n_rows != P) return mpcx_fail(ctx, MPCX_E_INVALID, "intent: n_rows = %d is not P = %d", s->n_rows, P);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "intent: not in the agent-sharded layout (the other ranks' rows arrive without their plans)");
    if (pool_rows < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "intent: no pool (a plan is shared through the agent's own pool row)");
    if (!obs_skip) return mpcx_fail(ctx, MPCX_E_INVALID, "intent: needs obs_skip (the agents' own pool rows)");
    if (P <= 0) return MPCX_OK;
    std::vector<int32_t> rows((size_t)P);
    if (hipMemcpy(rows.data(), obs_skip, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "intent: cannot read the agents' pool rows back for their check");
    for (int32_t q = 0; q < P; q++)
        if (rows[q] < 0 || rows[q] >= pool_rows)
            return mpcx_fail(ctx, MPCX_E_INVALID, "intent: agent %d has own pool row obs_skip = %d outside the pool of %d", q, rows[q], pool_rows);
    return MPCX_OK;
}

// the launch alone (the struct has been checked, ctx->pred holds the prediction of n_obs_pool rows): what mpcx_interaction_enqueue puts
// between the prediction and the conflict search, also inside a capture
int32_t mpcx_intent_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *obs_skip,
                            int32_t n_obs_pool, const mpcx_intent_launch &x) {
    mpcx::IntentArgs a;
    memset(&a, 0, sizeof a);
    a.ip = *ip;
    a.P = P; a.T = ctx->mpc.T; a.n_pool = n_obs_pool;
    a.has_done = x.done != nullptr; a.has_absent = x.absent != nullptr;
    a.state = state; a.u_sol = x.u_sol; a.status = x.status; a.obs_skip = obs_skip; a.done = x.done; a.absent = x.absent;
    a.pred = ctx->pred;
    a.in = x.in;
    const int per_block = mpcx::INT_WAVES * mpcx::INT_AGENTS;
    hipLaunchKernelGGL(mpcx::intent_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::INT_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "intent_kernel");
}

extern "C" int32_t mpcx_interaction_batch_intent(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state,
                                                 const double *path_xyyaw, const double *path_cs, const int32_t *path_off,
                                                 const int32_t *path_len, const int32_t *prev_cut_len, int32_t n_obs_pool, const double *obs6,
                                                 const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip, int32_t *traj_idx,
                                                 int32_t *hit_idx, double *hit_xy, int32_t *cut_len, const double *u_sol, const int32_t *status,
                                                 const int32_t *done, const int32_t *absent, const mpcx_intent *intent) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (P < 0 || n_obs_pool < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch_intent: negative size");
    int32_t rc = mpcx_intent_validate(ctx, intent, P, 0, obs6 ? n_obs_pool : 0, obs_skip);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!u_sol || !status) return mpcx_fail(ctx, MPCX_E_INVALID, "interaction_batch_intent: null buffer (u_sol, status)");
    mpcx_intent_launch il;
    il.u_sol = u_sol; il.status = status; il.done = done; il.absent = absent; il.in = *intent;
    mpcx_interaction_extras x;
    x.intent = &il;
    return mpcx_interaction_enqueue(ctx, ip, P, state, path_xyyaw, path_cs, path_off, path_len, prev_cut_len, n_obs_pool, obs6, obs_off, obs_cnt,
                                    obs_skip, traj_idx, hit_idx, hit_xy, cut_len, x);
}
