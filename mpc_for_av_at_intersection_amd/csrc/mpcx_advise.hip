// mpcx_advise.hip -- signal-aware approach speed in the device-resident closed loop: the struct's checks and the stage that caps the speed
// reference of an agent that would reach its stop line on red.  The rule is mpcx_advise_core.h.
// advise_kernel: one launch between the window stage and the QP, in speed mode under a fixed plan.  Laid out as part 3 of
// ref_window_kernel: a wavefront takes ADV_AGENTS consecutive agents (a block is ADV_WAVES wavefronts).  Lane i < ADV_AGENTS evaluates
// the rule of agent b0 + i once -- integers, one ceil, two divisions -- and writes advised[b0 + i]: one coalesced store.  Then the clamp,
// floor(64 / (T + 1)) agents per pass, each on a run of T + 1 lanes of its own that takes the agent's speed by a shuffle and does row 2 of
// its xref as one coalesced read-modify-write.  A wavefront none of whose agents is advised (most of them, most of the time) leaves after
// the store; a pass none of whose agents is advised is skipped: both conditions are wave-uniform.  Every access is to words of the
// wavefront's own agents plus the read-only tables.  No LDS, no scratch, no atomics.  Everything it reads is device memory, so a replayed
// hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_advise_core.h"
#include <cmath>
#include <cstring>

namespace mpcx {

constexpr int ADV_WAVES = 4;
constexpr int ADV_AGENTS = 16;
static_assert(ADV_AGENTS <= WAVE, "one lane per agent for the rule");

__global__ __launch_bounds__(64 * ADV_WAVES) void advise_kernel(AdviseArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = a.W;
    const int b0 = ((int)blockIdx.x * ADV_WAVES + wave) * ADV_AGENTS;
    const int nag = a.P - b0 < ADV_AGENTS ? a.P - b0 : ADV_AGENTS;      // agents of this wavefront (<= 0: none)
    if (nag <= 0) return;
    // ---- the rule: lane i < nag holds agent b0 + i
    double v = 0.0;
    if (lane < nag) {
        v = advise_speed(a, b0 + lane);
        a.ad.advised[b0 + lane] = v;
    }
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
        if (cap) advise_clamp(a, b0 + i, t, vi);
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no advice"
bool mpcx_advice_absent(const mpcx_advice *s) {
    return !s || (!s->advised && s->v_cruise == 0.0 && s->v_min == 0.0 && s->reach == 0.0 && s->lead == 0 && s->n_rows == 0);
}

// the struct's own fields and what advice needs of the run: signals under a fixed plan (which the caller checks by their own rule,
// mpcx_signals_validate), no controller, speed mode.  speed: the run's stop mode is MPCX_STOP_SPEED (a stage call vouches for it).  Never
// a GPU fault for a bad struct.
int32_t mpcx_advise_validate(mpcx_ctx *ctx, const mpcx_advice *s, const mpcx_signals *sg, bool actuated, bool speed, int32_t P) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "advice: null struct");
    if (!s->advised) return mpcx_fail(ctx, MPCX_E_INVALID, "advice: advised is null (n_rows doubles, one per agent)");
    if (s->n_rows != P) return mpcx_fail(ctx, MPCX_E_INVALID, "advice: n_rows = %d is not P = %d", s->n_rows, P);
    if (!std::isfinite(s->v_cruise) || !(s->v_cruise > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "advice: v_cruise = %g must be finite and positive", s->v_cruise);
    if (!std::isfinite(s->v_min) || !(s->v_min > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "advice: v_min = %g must be finite and positive", s->v_min);
    if (!std::isfinite(s->reach) || !(s->reach > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "advice: reach = %g must be finite and positive", s->reach);
    if (s->v_min > s->v_cruise) return mpcx_fail(ctx, MPCX_E_INVALID, "advice: v_min = %g > v_cruise = %g", s->v_min, s->v_cruise);
    if (s->lead < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "advice: lead = %d is negative", s->lead);
    if (mpcx_signals_absent(sg)) return mpcx_fail(ctx, MPCX_E_INVALID, "advice: needs signals (mpcx_signals supplies the stop lines, the plan and the clock)");
    if (actuated)
        return mpcx_fail(ctx, MPCX_E_INVALID, "advice: not with actuation (a controller decides the lights step by step: there is no plan to look ahead into)");
    if (!sg->plan_cycle || !sg->plan_green || !sg->plan_of || !sg->tick || sg->n_plans < 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "advice: the signals carry no fixed plan (plan_cycle, plan_green, plan_of, tick, n_plans >= 1): there is no plan to look ahead into");
    if (!speed)
        return mpcx_fail(ctx, MPCX_E_INVALID, "advice: the stop mode is not MPCX_STOP_SPEED (in cut mode the speed reference is 0: the stage would do nothing)");
    return MPCX_OK;
}

// the launch alone (the structs have been checked): what the closed loop enqueues behind the window stage, also inside a capture
int32_t mpcx_advise_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                            const int32_t *cut_len, const int32_t *done, const mpcx_signals *signals, const mpcx_advice *advice, double *xref) {
    mpcx::AdviseArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.W = ctx->mpc.T + 1; a.dl = dl; a.dt = ctx->mpc.dt;
    a.path_off = path_off; a.path_len = path_len; a.traj_idx = traj_idx; a.cut_len = cut_len; a.done = done; a.xref = xref;
    a.sg = *signals; a.ad = *advice;
    const int per_block = mpcx::ADV_WAVES * mpcx::ADV_AGENTS;
    hipLaunchKernelGGL(mpcx::advise_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::ADV_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "advise_kernel");
}

extern "C" int32_t mpcx_advise_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const int32_t *path_off, const int32_t *path_len,
                                          const int32_t *traj_idx, const int32_t *cut_len, const int32_t *done, const mpcx_signals *signals,
                                          const mpcx_advice *advice, double *xref) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "advise_step_batch: negative size");
    int32_t rc = mpcx_advise_validate(ctx, advice, signals, false, true, P);
    if (rc == MPCX_OK) rc = mpcx_signals_validate(ctx, signals, 0);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!path_off || !path_len || !traj_idx || !cut_len || !xref || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "advise_step_batch: null buffer (path_off, path_len, traj_idx, cut_len, xref) or dl <= 0");
    return mpcx_advise_enqueue(ctx, P, dl, path_off, path_len, traj_idx, cut_len, done, signals, advice, xref);
}
