// mpcx_brake.hip -- firm hold in the device-resident closed loop: the struct's checks, the setter that attaches it to the context and the two
// launches.  The rule is mpcx_brake_core.h.
// brake_mark_kernel: one lane per agent, behind the last hold stage and the following stage, in front of the window stage, in both stop
// modes.  It does the line-held test, writes firm and, in speed mode, clamps the window's start index and writes the per-agent length the
// window stage is handed in place of path_len.
// brake_clamp_kernel has the shape of follow_clamp_kernel: lane i of a wavefront looks at agent b0 + i -- its firm word, its line, its stop
// point -- and does what belongs to the agent alone (the pin, overran, brake_cap from window point 0, prev_len); then floor(64 / (T + 1))
// agents per pass, each on a run of T + 1 lanes of its own, take the profile, one window point per lane, with the stop point handed over by
// shuffle.  A wavefront or a pass without a line-held agent is skipped, both conditions wave-uniform.  The agent's lane reads window point
// 0's position only, which no lane writes, so no lane reads a word another lane writes.  No LDS, no scratch, no atomics; everything either
// kernel reads is device memory, so a replayed hipGraph behaves like a plain run.
#include "mpcx_common.h"
#include "mpcx_brake_core.h"
#include <cmath>
#include <cstring>

namespace mpcx {

constexpr int BRAKE_WAVES = 4;
constexpr int BRAKE_CLAMP_AGENTS = 16;

__global__ __launch_bounds__(64 * BRAKE_WAVES) void brake_mark_kernel(BrakeArgs a) {
    const int q = (int)(blockIdx.x * (unsigned)(64 * BRAKE_WAVES) + threadIdx.x);
    if (q >= a.P) return;
    brake_mark_agent(a, q);
}

__global__ __launch_bounds__(64 * BRAKE_WAVES) void brake_clamp_kernel(BrakeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = a.W;
    const int b0 = ((int)blockIdx.x * BRAKE_WAVES + wave) * BRAKE_CLAMP_AGENTS;
    const int nag = a.P - b0 < BRAKE_CLAMP_AGENTS ? a.P - b0 : BRAKE_CLAMP_AGENTS;        // agents of this wavefront (<= 0: none)
    if (nag <= 0) return;
    // ---- the agent's own lane: its line, and the words that belong to the agent alone
    BrakeLine l{0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool held = lane < nag && brake_clamp_line(a, b0 + lane, &l);
    if (__ballot(held) == 0) return;
    if (held) brake_clamp_words(a, b0 + lane, l);
    // ---- the profile: lane = (agent g of the pass, window point t)
    const int G = 64 / W;
    const int g = lane / W, t = lane - g * W;
    for (int base = 0; base < nag; base += G) {
        const int i = base + g;
        const bool on = g < G && i < nag;
        const int from = on ? i : 0;
        const bool hi = __shfl((int)held, from) != 0;
        const double ex = __shfl(l.ex, from), ey = __shfl(l.ey, from);
        const bool cap = on && hi;
        if (__ballot(cap) == 0) continue;
        if (cap) brake_clamp_point(a, b0 + i, t, ex, ey);
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no firm hold"
bool mpcx_braking_absent(const mpcx_braking *s) {
    return !s || (!s->firm && !s->overran && !s->brake_cap && s->brake == 0.0 && s->setback == 0.0);
}

// the struct's own fields and what the stage needs of the run.  exchange: the descriptor's (0 for a stage call); lin_passes: the context's
// (1 for a stage call); lines: the run has a source of stop lines.  Never a GPU fault for a bad struct.
int32_t mpcx_braking_validate(mpcx_ctx *ctx, const mpcx_braking *s, double dl, int32_t exchange, int32_t lin_passes, bool lines) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "braking: null struct");
    const char *missing = !s->firm ? "firm" : !s->overran ? "overran" : !s->brake_cap ? "brake_cap" : nullptr;
    if (missing) return mpcx_fail(ctx, MPCX_E_INVALID, "braking: %s is null (firm, overran and brake_cap: one word per agent)", missing);
    if (!std::isfinite(s->brake) || !(s->brake > 0.0)) return mpcx_fail(ctx, MPCX_E_INVALID, "braking: brake = %g must be finite and positive", s->brake);
    if (!std::isfinite(s->setback) || !(dl > 0.0) || !(s->setback >= 2.0 * dl))
        return mpcx_fail(ctx, MPCX_E_INVALID, "braking: setback = %g must be finite and at least 2 dl = %g (the pin needs two points between the stop point and the line)",
                         s->setback, 2.0 * dl);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "braking: not supported in the agent-sharded layout (shard by instances)");
    if (lin_passes != 1) return mpcx_fail(ctx, MPCX_E_INVALID, "braking: not supported with more than one linearisation pass (%d)", lin_passes);
    if (!lines)
        return mpcx_fail(ctx, MPCX_E_INVALID, "braking: the run has no source of stop lines (signals, actuation, a reservation, the priority road or stop signs)");
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_braking(mpcx_ctx *ctx, const mpcx_braking *s) {
    if (!ctx) return MPCX_E_INVALID;
    memset(&ctx->braking, 0, sizeof ctx->braking);
    ctx->have_braking = !mpcx_braking_absent(s);
    if (ctx->have_braking) {
        mpcx_braking &b = ctx->braking;
        b.brake = s->brake; b.setback = s->setback; b.firm = s->firm; b.overran = s->overran; b.brake_cap = s->brake_cap;
    }
    return MPCX_OK;
}

static mpcx::BrakeArgs brake_args(int32_t P, int32_t W, bool speed, double dl, const int32_t *path_off, const int32_t *path_len,
                                  int32_t *traj_idx, const int32_t *done, const int32_t *path_stop, int32_t n_points, const mpcx_braking *braking) {
    mpcx::BrakeArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.W = W; a.speed = speed ? 1 : 0; a.dl = dl;
    a.path_off = path_off; a.path_len = path_len; a.traj_idx = traj_idx; a.done = done; a.path_stop = path_stop; a.n_points = n_points;
    a.br = *braking;
    return a;
}

// the launches alone (the struct has been checked): what the closed loop enqueues, also inside a capture
int32_t mpcx_brake_mark_enqueue(mpcx_ctx *ctx, int32_t P, double dl, bool speed, const int32_t *path_off, const int32_t *path_len,
                                const int32_t *traj_idx, int32_t *target_ind, int32_t *win_len, const int32_t *done, const int32_t *path_stop,
                                int32_t n_points, const int32_t *held, const int32_t *boxed, const int32_t *yielding, const mpcx_braking *braking) {
    mpcx::BrakeArgs a = brake_args(P, 0, speed, dl, path_off, path_len, const_cast<int32_t *>(traj_idx) /* read only here */, done, path_stop, n_points, braking);
    a.target_ind = target_ind; a.win_len = win_len; a.held = held; a.boxed = boxed; a.yielding = yielding;
    const int per_block = 64 * mpcx::BRAKE_WAVES;
    hipLaunchKernelGGL(mpcx::brake_mark_kernel, dim3((P + per_block - 1) / per_block), dim3(per_block), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "brake_mark_kernel");
}

int32_t mpcx_brake_clamp_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const double *path_xyyaw, const int32_t *path_off,
                                 const int32_t *path_len, int32_t *traj_idx, int32_t *len_seen, const int32_t *done, const int32_t *path_stop,
                                 int32_t n_points, const mpcx_braking *braking, double *xref) {
    mpcx::BrakeArgs a = brake_args(P, ctx->mpc.T + 1, true, dl, path_off, path_len, traj_idx, done, path_stop, n_points, braking);
    a.state = state; a.path_xyyaw = path_xyyaw; a.len_seen = len_seen; a.xref = xref;
    const int per_block = mpcx::BRAKE_WAVES * mpcx::BRAKE_CLAMP_AGENTS;
    hipLaunchKernelGGL(mpcx::brake_clamp_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::BRAKE_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "brake_clamp_kernel");
}

extern "C" int32_t mpcx_brake_mark_step_batch(mpcx_ctx *ctx, int32_t P, double dl, int32_t stop_mode, const int32_t *path_off, const int32_t *path_len,
                                              const int32_t *traj_idx, int32_t *target_ind, int32_t *win_len, const int32_t *done,
                                              const int32_t *path_stop, int32_t n_points, const int32_t *held, const int32_t *boxed,
                                              const int32_t *yielding, const mpcx_braking *braking) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0 || n_points < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "brake_mark_step_batch: negative size");
    if (stop_mode != MPCX_STOP_CUT && stop_mode != MPCX_STOP_SPEED)
        return mpcx_fail(ctx, MPCX_E_INVALID, "brake_mark_step_batch: unknown stop mode %d (MPCX_STOP_CUT or MPCX_STOP_SPEED)", stop_mode);
    const int32_t rc = mpcx_braking_validate(ctx, braking, dl, 0, 1, path_stop && (held || boxed || yielding));
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!path_off || !path_len || !traj_idx) return mpcx_fail(ctx, MPCX_E_INVALID, "brake_mark_step_batch: null buffer (path_off, path_len, traj_idx)");
    if (stop_mode == MPCX_STOP_SPEED && (!target_ind || !win_len))
        return mpcx_fail(ctx, MPCX_E_INVALID, "brake_mark_step_batch: MPCX_STOP_SPEED needs target_ind and win_len");
    return mpcx_brake_mark_enqueue(ctx, P, dl, stop_mode == MPCX_STOP_SPEED, path_off, path_len, traj_idx, target_ind, win_len, done, path_stop, n_points,
                                   held, boxed, yielding, braking);
}

extern "C" int32_t mpcx_brake_clamp_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const double *path_xyyaw,
                                               const int32_t *path_off, const int32_t *path_len, int32_t *traj_idx, int32_t *prev_len,
                                               const int32_t *done, const int32_t *path_stop, int32_t n_points, const mpcx_braking *braking,
                                               double *xref) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (P < 0 || n_points < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "brake_clamp_step_batch: negative size");
    const int32_t rc = mpcx_braking_validate(ctx, braking, dl, 0, 1, path_stop != nullptr);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_xyyaw || !path_off || !path_len || !traj_idx || !xref)
        return mpcx_fail(ctx, MPCX_E_INVALID, "brake_clamp_step_batch: null buffer (state, path_xyyaw, path_off, path_len, traj_idx, xref)");
    return mpcx_brake_clamp_enqueue(ctx, P, dl, state, path_xyyaw, path_off, path_len, traj_idx, prev_len, done, path_stop, n_points, braking, xref);
}
