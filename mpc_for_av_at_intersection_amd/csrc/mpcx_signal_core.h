// mpcx_signal_core.h -- TRAFFIC SIGNALS: an agent whose light is red (or amber, if it can stop) is held at its stop line.  Host + device
// source (the pattern of mpcx_admit_core.h, mpcx_route_core.h and mpcx_precedence_core.h).  signal_kernel (mpcx_signal.hip) runs it one
// lane per agent directly after the conflict search of a closed-loop step; tests/signal_ref/signal_ref.cpp builds it for the host.
//
// The reference holds an ego by ending its path in front of a conflict (tmp_trajectory = trajectory_full[:cutoff_idx]); a red light is a
// conflict at a known point of the agent's own path.  The rule shortens cut_len (the cut length, or the stop index in speed mode) and
// nothing else: the window stage, the QP, the run log, the goal test and the "do not advance traj_agent_idx on the path end" rule follow.
//
// Stop lines belong to PATH POINTS: path_stop[i] is the route-local index s of the next stop-line point at or after absolute path point i
// (-1: none ahead), path_group[i] that line's signal group.  Routes that change per vehicle (mpcx_routes) need nothing extra.
// Plans: plan_cycle[n_plans] (steps, >= 1), plan_amber[n_plans] (steps, >= 0), plan_green[n_plans][n_groups][2] = (green_from, green_len),
// plan_of[P] the plan of agent q.  The clock is one word per agent, tick[P]: a per-instance offset is its initial value.
// Light of group g at t in [0, cycle): u = t - green_from (+ cycle if negative); GREEN if u < green_len, AMBER if u < green_len + amber,
// RED otherwise.  Integers only.
//
// For agent q, in this order:
//   1. t = tick[q] reduced into [0, cycle), tick[q] = t + 1 wrapped at cycle -- every step, whether the agent drives or not.  (An agent
//      whose plan_of is out of range, or whose plan has cycle < 1, has no cycle: its tick is left alone and it is free, 3.)
//   2. done[q] != 0 (retirement): held[q] = 0, nothing else is touched.
//   3. i = path_off[q] + traj_idx[q] (traj_idx as this step's conflict search left it), s = path_stop[i], g = path_group[i].  Free,
//      held[q] = 0: no line ahead (s < 0); on or past the line (traj_idx[q] >= s); a defective entry -- i outside [0, n_points), g or
//      plan_of[q] out of range, s >= path_len[q].
//   4. else the light: GREEN free; RED held[q] = 1; AMBER held[q] = 2 if held[q] was nonzero already (the decision in amber is sticky: a
//      car that began to brake does not change its mind) or if it can stop, (s - traj_idx[q]) * dl >= v * v / (2 * brake), v = state[q][2];
//      else free.  held is in-out, zero-initialised by the caller.
//   5. held: cut_len[q] = min(cut_len[q], s).  traj_idx < s, so this is the reference's max(traj_agent_idx + 1, cutoff_idx): the path ends
//      on the point before the line.  A conflict cut shorter than s is kept.
// The text is in two parts: signal_agent is step 1, "clock and light"; signal_hold is steps 2 - 5, the hold, which takes the light of a group
// from its caller and is shared with the vehicle-actuated rule (mpcx_actuated_core.h), where a junction's controller supplies the light.
// Every access is to words of agent q plus the read-only tables: no lane reads a word another lane writes, the outcome does not depend on
// the order of the lanes, and a replayed hipGraph counts like a plain run.  The stopping distance has no multiply-add to fuse; host builds
// use -ffp-contract=off all the same.
#pragma once
#include "mpcx_record_core.h"

#define MPCX_SIGNAL_GREEN 0
#define MPCX_SIGNAL_AMBER 1
#define MPCX_SIGNAL_RED 2

#ifdef __HIPCC__
#define MPCX_REC_FN_MEMBER __host__ __device__ __forceinline__
#else
#define MPCX_REC_FN_MEMBER inline
#endif

namespace mpcx {

struct SignalArgs {
    int P;
    double dl;
    const double *state;                    // P x 4
    const int32_t *path_off, *path_len;     // P each
    const int32_t *traj_idx;                // P, as the conflict search left it
    int32_t *cut_len;                       // P, in-out
    const int32_t *done;                    // P or nullptr
    mpcx_signals sg;
};

// the light of a group with (green_from, green_len) at t in [0, cycle)
MPCX_REC_FN int signal_light(int32_t cycle, int32_t amber, int32_t green_from, int32_t green_len, int32_t t) {
    int32_t u = t - green_from;
    if (u < 0) u += cycle;
    if (u < green_len) return MPCX_SIGNAL_GREEN;
    if (u < green_len + amber) return MPCX_SIGNAL_AMBER;
    return MPCX_SIGNAL_RED;
}

// the light of agent q's group under a fixed plan at t (the "clock and light" half of the rule hands this to the hold)
struct PlanLight {
    const mpcx_signals *g;
    int32_t plan, cycle, t;
    MPCX_REC_FN_MEMBER int operator()(int32_t grp) const {
        const int32_t *gr = g->plan_green + 2 * ((size_t)plan * (size_t)g->n_groups + (size_t)grp);
        return signal_light(cycle, g->plan_amber[plan], gr[0], gr[1], t);
    }
};

// steps 2 - 5, THE HOLD, shared by the fixed-time rule and the actuated one (mpcx_actuated_core.h): lit = the agent has a source of light
// at all (a cycle, a controller), light_of(grp) the light of signal group grp in this step.  Returns held[q] as it is left.
template <class LightOf>
MPCX_REC_FN int32_t signal_hold(const SignalArgs &a, int q, bool lit, const LightOf &light_of) {
    const mpcx_signals &g = a.sg;
    if (a.done && a.done[q] != 0) { g.held[q] = 0; return 0; }
    const int32_t ti = a.traj_idx[q];
    const int64_t i = (int64_t)a.path_off[q] + (int64_t)ti;
    int32_t held = 0;
    if (lit && i >= 0 && i < (int64_t)g.n_points) {
        const int32_t s = g.path_stop[i], grp = g.path_group[i];
        if (s >= 0 && ti < s && s < a.path_len[q] && grp >= 0 && grp < g.n_groups) {
            const int light = light_of(grp);
            if (light == MPCX_SIGNAL_RED) held = 1;
            else if (light == MPCX_SIGNAL_AMBER) {
                const double v = a.state[4 * (size_t)q + 2];
                if (g.held[q] != 0 || (double)(s - ti) * a.dl >= v * v / (2.0 * g.brake)) held = 2;
            }
            if (held != 0 && s < a.cut_len[q]) a.cut_len[q] = s;
        }
    }
    g.held[q] = held;
    return held;
}

// step 1, CLOCK AND LIGHT, then the hold; returns held[q] as it is left
MPCX_REC_FN int32_t signal_agent(const SignalArgs &a, int q) {
    const mpcx_signals &g = a.sg;
    const int32_t plan = g.plan_of[q];
    const bool has_plan = plan >= 0 && plan < g.n_plans;
    const int32_t cycle = has_plan ? g.plan_cycle[plan] : 0;
    int32_t t = 0;
    if (cycle >= 1) {
        t = g.tick[q] % cycle;
        if (t < 0) t += cycle;
        g.tick[q] = t + 1 < cycle ? t + 1 : 0;
    }
    return signal_hold(a, q, cycle >= 1, PlanLight{&g, plan, cycle, t});
}

}  // namespace mpcx
