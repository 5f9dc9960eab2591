// mpcx_actuated.hip -- vehicle-actuated signals in the device-resident closed loop: the struct's checks and the stage that runs a
// controller per junction and holds the junction's agents at their stop lines.  The rule is mpcx_actuated_core.h; the hold is
// mpcx_signal_core.h's.
// actuated_signal_kernel: one launch in the place of signal_kernel, directly after the conflict search and before the window stage, in both
// stop modes.  A LANE GROUP of G lanes per junction, G the smallest power of two >= n_per capped at 64, 64 / G junctions per wavefront (a
// block is one wavefront); a lane takes agents lane, lane + G, ... of its junction, so n_per > 64 is one wavefront striding.  Each lane ORs
// its agents' call bits, a butterfly of __shfl_xor within the group gives every lane the junction's calls, every lane reads jstate and runs
// the state machine redundantly (a few dozen integer operations on uniform words: cheaper than a broadcast), the group's first lane
// writes jstate, lights and calls, then every lane applies the hold to its own agents.  All lanes of a group sit in one wavefront and the
// reads of jstate stand before the write in program order, so no lane reads a word another lane of the launch writes.  No LDS, no
// scratch, no atomics.  Everything it reads is device memory, so a replayed hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_actuated_core.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mpcx {

template <int G>
__global__ __launch_bounds__(64) void actuated_signal_kernel(ActuatedArgs a) {
    const mpcx_actuation &c = a.ac;
    const int sub = threadIdx.x & (G - 1);
    const int j = blockIdx.x * (64 / G) + (threadIdx.x / G);
    const bool live = j < c.n_junctions;        // (a dead group stays for the butterfly: no lane leaves early)
    const int q0 = live ? j * c.n_per : 0;
    const int32_t k = live ? actuated_ctrl(c, j) : -1;
    uint32_t lights = 0, calls = 0;
    JunctionWord s{0, 0, 0, 0};
    int32_t detect = 0;
    if (k >= 0) {
        s = actuated_read(c, j);
        lights = actuated_lights((uint32_t)c.phase_groups[(size_t)k * (size_t)c.n_phases + (size_t)s.phase], s.stage, a.s.sg.n_groups);
        detect = c.ctrl_time[3 * (size_t)k + 2];
        for (int r = sub; r < c.n_per; r += G) calls |= actuated_call(a.s, q0 + r, detect);
    }
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) calls |= (uint32_t)__shfl_xor((int)calls, m, G);
    if (k >= 0) {
        const JunctionWord t = actuated_advance(c, k, s, calls);
        if (sub == 0) {
            int32_t *w = c.jstate + 4 * (size_t)j;
            w[0] = t.phase; w[1] = t.stage; w[2] = t.timer; w[3] = t.idle;
        }
    }
    if (live && sub == 0) {
        c.lights[j] = (int32_t)lights;
        c.calls[j] = (int32_t)calls;
    }
    if (live)
        for (int r = sub; r < c.n_per; r += G) (void)signal_hold(a.s, q0 + r, k >= 0, WordLight{lights});
}

}  // namespace mpcx

// all-zero (or no) struct: "no actuation"
bool mpcx_actuation_absent(const mpcx_actuation *s) {
    return !s || (!s->phase_groups && !s->phase_time && !s->ctrl_time && !s->ctrl_of && !s->jstate && !s->lights && !s->calls && s->n_per == 0 &&
                  s->n_junctions == 0 && s->n_phases == 0 && s->n_ctrl == 0 && s->reserved == 0);
}

// the two structs' own fields and what actuation needs of the run; reads the three controller tables back (never inside a capture).
// exchange: the descriptor's (0 for a stage call).  Never a GPU fault for a bad struct.
int32_t mpcx_actuation_validate(mpcx_ctx *ctx, const mpcx_actuation *s, const mpcx_signals *sg, int32_t P, int32_t exchange) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: null struct");
    if (!sg) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: needs signals (mpcx_signals supplies the stop lines, held and brake)");
    if (sg->plan_cycle || sg->plan_amber || sg->plan_green || sg->plan_of || sg->tick || sg->n_plans != 0)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: the signals also carry a fixed plan (plan_cycle, plan_amber, plan_green, plan_of and tick must be null, n_plans 0): one source of lights");
    const char *missing = !sg->path_stop ? "signals.path_stop" : !sg->path_group ? "signals.path_group" : !sg->held ? "signals.held" :
                          !s->phase_groups ? "phase_groups" : !s->phase_time ? "phase_time" : !s->ctrl_time ? "ctrl_time" : !s->ctrl_of ? "ctrl_of" :
                          !s->jstate ? "jstate" : !s->lights ? "lights" : !s->calls ? "calls" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: %s is null (phase_groups, phase_time, ctrl_time, ctrl_of, jstate, lights, calls and the signals' path_stop, path_group and held are all required)", missing);
    if (sg->n_groups < 1 || sg->n_groups > MPCX_SIGNAL_GROUPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: signals.n_groups = %d outside 1..%d", sg->n_groups, MPCX_SIGNAL_GROUPS_MAX);
    if (sg->n_points < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: signals.n_points = %d, at least one path point", sg->n_points);
    if (!std::isfinite(sg->brake) || !(sg->brake > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: signals.brake = %g must be finite and positive", sg->brake);
    if (sg->reserved != 0 || s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: a reserved word is not 0");
    if (s->n_per < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: n_per = %d, at least one agent per junction", s->n_per);
    if (s->n_junctions < 0 || (int64_t)s->n_per * (int64_t)s->n_junctions != (int64_t)P)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: n_per * n_junctions = %d * %d is not P = %d", s->n_per, s->n_junctions, P);
    if (s->n_phases < 1 || s->n_phases > MPCX_ACTUATION_PHASES_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: n_phases = %d outside 1..%d", s->n_phases, MPCX_ACTUATION_PHASES_MAX);
    if (s->n_ctrl < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: n_ctrl = %d, at least one controller", s->n_ctrl);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: not supported in the agent-sharded layout (shard by instances)");
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: %d linearisation passes; the signal stage sits in front of a single window stage", ctx->lin_passes);
    const size_t nc = (size_t)s->n_ctrl, np = (size_t)s->n_phases;
    std::vector<int32_t> grp(nc * np), pt(3 * nc * np), ct(3 * nc);
    if (hipMemcpy(grp.data(), s->phase_groups, grp.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pt.data(), s->phase_time, pt.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ct.data(), s->ctrl_time, ct.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "actuation: cannot read the controller tables back for their check");
    const uint32_t all = sg->n_groups >= 32 ? ~0u : (1u << sg->n_groups) - 1u;
    for (size_t k = 0; k < nc; k++) {
        for (size_t p = 0; p < np; p++) {
            const uint32_t m = (uint32_t)grp[k * np + p];
            const int32_t mn = pt[3 * (k * np + p)], mx = pt[3 * (k * np + p) + 1], gap = pt[3 * (k * np + p) + 2];
            if (m == 0 || (m & ~all) != 0)
                return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d phase %d has group mask = 0x%x (nonzero, bits below n_groups = %d)", (int)k, (int)p, m, sg->n_groups);
            if (mn < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d phase %d has min_green = %d", (int)k, (int)p, mn);
            if (mx < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d phase %d has max_green = %d (at least 1 step)", (int)k, (int)p, mx);
            if (mn > mx) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d phase %d has min_green = %d > max_green = %d", (int)k, (int)p, mn, mx);
            if (gap < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d phase %d has gap = %d (at least 1 step)", (int)k, (int)p, gap);
        }
        if (ct[3 * k] < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d has amber = %d", (int)k, ct[3 * k]);
        if (ct[3 * k + 1] < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d has all_red = %d", (int)k, ct[3 * k + 1]);
        if (ct[3 * k + 2] < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "actuation: controller %d has detect = %d (at least 1 path point)", (int)k, ct[3 * k + 2]);
    }
    return MPCX_OK;
}

// the launch alone (the structs have been checked): what the closed loop enqueues behind the conflict search, also inside a capture
int32_t mpcx_actuated_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                              const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const mpcx_signals *signals,
                              const mpcx_actuation *actuation) {
    mpcx::ActuatedArgs a;
    memset(&a, 0, sizeof a);
    a.s = mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, *signals};
    a.ac = *actuation;
    const int J = actuation->n_junctions, n = actuation->n_per;
    if (J == 0) return MPCX_OK;
#define MPCX_ACT_LAUNCH(G) hipLaunchKernelGGL(mpcx::actuated_signal_kernel<G>, dim3((J + 64 / G - 1) / (64 / G)), dim3(64), 0, ctx->stream, a)
    if (n <= 1) MPCX_ACT_LAUNCH(1);
    else if (n <= 2) MPCX_ACT_LAUNCH(2);
    else if (n <= 4) MPCX_ACT_LAUNCH(4);
    else if (n <= 8) MPCX_ACT_LAUNCH(8);
    else if (n <= 16) MPCX_ACT_LAUNCH(16);
    else if (n <= 32) MPCX_ACT_LAUNCH(32);
    else MPCX_ACT_LAUNCH(64);
#undef MPCX_ACT_LAUNCH
    return mpcx_check_launch(ctx, "actuated_signal_kernel");
}

extern "C" int32_t mpcx_actuated_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off,
                                            const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                                            const mpcx_signals *signals, const mpcx_actuation *actuation) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "actuated_step_batch: negative size");
    const int32_t rc = mpcx_actuation_validate(ctx, actuation, signals, P, 0);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !path_len || !traj_idx || !cut_len || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "actuated_step_batch: null buffer (state, path_off, path_len, traj_idx, cut_len) or dl <= 0");
    return mpcx_actuated_enqueue(ctx, P, dl, state, path_off, path_len, traj_idx, cut_len, done, signals, actuation);
}
