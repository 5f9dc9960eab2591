// mpcx_signal.hip -- traffic signals in the device-resident closed loop: the struct's checks and the stage that holds agents at their stop
// lines.  The rule is mpcx_signal_core.h.
// signal_kernel: one launch directly after the conflict search and before the window stage, in both stop modes; one lane per agent.  A lane
// loads its agent's plan words once, advances the agent's clock and, where the light holds the agent, shortens its cut length (its stop
// index in speed mode).  Every access is to words of agent q plus the read-only tables.  No LDS, no scratch.  Everything it reads is
// device memory, so a replayed hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_signal_core.h"
#include <cmath>
#include <vector>

namespace mpcx {

__global__ __launch_bounds__(64) void signal_kernel(SignalArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    (void)signal_agent(a, q);
}

}  // namespace mpcx

// all-zero (or no) struct: "no signals"
bool mpcx_signals_absent(const mpcx_signals *s) {
    return !s || (!s->path_stop && !s->path_group && !s->plan_cycle && !s->plan_amber && !s->plan_green && !s->plan_of && !s->tick && !s->held &&
                  s->brake == 0.0 && s->n_points == 0 && s->n_plans == 0 && s->n_groups == 0 && s->reserved == 0);
}

// the struct's own fields and what signals need of the run; reads the three plan tables back (never inside a capture).  exchange: the
// descriptor's (0 for a stage call).  Never a GPU fault for a bad struct.
int32_t mpcx_signals_validate(mpcx_ctx *ctx, const mpcx_signals *s, int32_t exchange) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "signals: null struct");
    const char *missing = !s->path_stop ? "path_stop" : !s->path_group ? "path_group" : !s->plan_cycle ? "plan_cycle" : !s->plan_amber ? "plan_amber" :
                          !s->plan_green ? "plan_green" : !s->plan_of ? "plan_of" : !s->tick ? "tick" : !s->held ? "held" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "signals: path_stop, path_group (n_points), plan_cycle, plan_amber (n_plans), plan_green (n_plans, n_groups, 2), plan_of, tick and held (P) are all required, %s is null", missing);
    if (s->n_groups < 1 || s->n_groups > MPCX_SIGNAL_GROUPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "signals: n_groups = %d outside 1..%d", s->n_groups, MPCX_SIGNAL_GROUPS_MAX);
    if (s->n_plans < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "signals: n_plans = %d, at least one plan", s->n_plans);
    if (s->n_points < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "signals: n_points = %d, at least one path point", s->n_points);
    if (!std::isfinite(s->brake) || !(s->brake > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "signals: brake = %g must be finite and positive", s->brake);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "signals: not supported in the agent-sharded layout (shard by instances)");
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "signals: %d linearisation passes; the signal stage sits in front of a single window stage", ctx->lin_passes);
    const size_t np = (size_t)s->n_plans, ng = (size_t)s->n_groups;
    std::vector<int32_t> cyc(np), amb(np), grn(2 * np * ng);
    if (hipMemcpy(cyc.data(), s->plan_cycle, np * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(amb.data(), s->plan_amber, np * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(grn.data(), s->plan_green, grn.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "signals: cannot read the plan tables back for their check");
    for (size_t p = 0; p < np; p++) {
        if (cyc[p] < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "signals: plan %d has cycle = %d (at least 1 step)", (int)p, cyc[p]);
        if (amb[p] < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "signals: plan %d has amber = %d", (int)p, amb[p]);
        for (size_t g = 0; g < ng; g++) {
            const int32_t from = grn[2 * (p * ng + g)], len = grn[2 * (p * ng + g) + 1];
            if (from < 0 || from >= cyc[p])
                return mpcx_fail(ctx, MPCX_E_INVALID, "signals: plan %d group %d has green_from = %d outside [0, %d)", (int)p, (int)g, from, cyc[p]);
            if (len < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "signals: plan %d group %d has green_len = %d", (int)p, (int)g, len);
            if ((int64_t)len + (int64_t)amb[p] > (int64_t)cyc[p])
                return mpcx_fail(ctx, MPCX_E_INVALID, "signals: plan %d group %d has green_len + amber = %d + %d > cycle = %d", (int)p, (int)g, len, amb[p], cyc[p]);
        }
    }
    return MPCX_OK;
}

// the launch alone (the struct has been checked): what the closed loop enqueues behind the conflict search, also inside a capture
int32_t mpcx_signal_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                            const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const mpcx_signals *signals) {
    const mpcx::SignalArgs a{P, dl, state, path_off, path_len, traj_idx, cut_len, done, *signals};
    hipLaunchKernelGGL(mpcx::signal_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "signal_kernel");
}

extern "C" int32_t mpcx_signal_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off,
                                          const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                                          const mpcx_signals *signals) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "signal_step_batch: negative size");
    const int32_t rc = mpcx_signals_validate(ctx, signals, 0);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !path_len || !traj_idx || !cut_len || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "signal_step_batch: null buffer (state, path_off, path_len, traj_idx, cut_len) or dl <= 0");
    return mpcx_signal_enqueue(ctx, P, dl, state, path_off, path_len, traj_idx, cut_len, done, signals);
}
