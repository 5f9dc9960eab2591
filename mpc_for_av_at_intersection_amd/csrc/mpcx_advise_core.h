// mpcx_advise_core.h -- SIGNAL-AWARE APPROACH SPEED: an agent that would reach its stop line on red at cruise speed is given the speed at
// which it reaches the line as the light turns green, as a cap on its speed reference.  Host + device source (the pattern of
// mpcx_signal_core.h, whose argument words and table layout it shares).  advise_kernel (mpcx_advise.hip) runs it between the window stage
// and the QP of a closed-loop step in speed mode; tests/advise_ref/advise_ref.cpp builds it for the host.
//
// In speed mode a red light zeroes the speed reference from the stop line on and leaves the path whole, so the position reference keeps
// pulling the car forward: it reaches the line at speed, brakes late and creeps over.  The plan is a table in device memory, so the agent
// can know when its light turns green.  The rule caps row 2 of the agent's xref (the speed reference over the window) and touches nothing
// else: the hold of mpcx_signal_core.h stays the safety net behind it.
//
// For agent q, reading traj_idx, cut_len, tick and held as the signal stage of this step left them:
//   1. NO ADVICE, advised[q] = 0.0 and xref untouched: done[q] != 0; no plan (plan_of[q] out of range) or cycle < 1; any "free" condition
//      of the hold -- with i = path_off[q] + traj_idx[q]: i outside [0, n_points), s = path_stop[i] < 0, traj_idx[q] >= s, s >= path_len[q],
//      the group out of range --; cut_len[q] < s (a conflict stops the agent before its line); d > reach, d = (double)(s - traj_idx[q]) * dl.
//   2. the clock: t0 = tick[q] - 1 (+ cycle if negative), the value the signal stage used this step.
//   3. earliest arrival: k_c = ceil(d / (v_cruise * dt)) as an integer clamped to 2^30; u = (t0 + k_c - green_from) mod cycle,
//      non-negative.  u < green_len: the agent arrives on green at cruise speed, no advice.
//   4. otherwise w = cycle - u steps of red are left at that arrival, k_t = k_c + w + lead, v = d / ((double)k_t * dt) and
//      advised[q] = max(v, v_min).
//   5. the clamp: every entry of row 2 of agent q's xref becomes min(entry, advised[q]); the zeros of the stop profile stay zero.
// Integers, one ceil, two divisions, one product in front of each division: nothing a compiler could fuse (contraction is switched off all
// the same) and every operation correctly rounded on host and device, so the two agree bit for bit.  Every access is to words of agent q
// plus the read-only tables: no lane reads a word another lane writes and the outcome does not depend on the order of the lanes.  A held
// agent IS advised.
#pragma once
#include <math.h>
#include "mpcx_signal_core.h"

#if defined(__clang__)
#define MPCX_ADV_NO_CONTRACT _Pragma("clang fp contract(off)")
#else       /* g++ honours no such pragma: a host build with it passes -ffp-contract=off */
#define MPCX_ADV_NO_CONTRACT
#endif

namespace mpcx {

constexpr int32_t ADVISE_STEPS_MAX = 1 << 30;       // the clamp of k_c

struct AdviseArgs {
    int P, W;                               // agents; window points T + 1
    double dl, dt;                          // path spacing; the MPC's time step
    const int32_t *path_off, *path_len;     // P each
    const int32_t *traj_idx, *cut_len;      // P each, as the signal stage left them
    const int32_t *done;                    // P or nullptr
    double *xref;                           // P x 4 x W, row 2 of every agent is clamped in place
    mpcx_signals sg;
    mpcx_advice ad;
};

// steps 1 - 4: the advised speed of agent q, 0.0 = none.  Reads only.
MPCX_REC_FN double advise_speed(const AdviseArgs &a, int q) {
    MPCX_ADV_NO_CONTRACT
    const mpcx_signals &g = a.sg;
    if (a.done && a.done[q] != 0) return 0.0;
    const int32_t plan = g.plan_of[q];
    if (plan < 0 || plan >= g.n_plans) return 0.0;
    const int32_t cycle = g.plan_cycle[plan];
    if (cycle < 1) return 0.0;
    const int32_t ti = a.traj_idx[q];
    const int64_t i = (int64_t)a.path_off[q] + (int64_t)ti;
    if (i < 0 || i >= (int64_t)g.n_points) return 0.0;
    const int32_t s = g.path_stop[i], grp = g.path_group[i];
    if (s < 0 || ti >= s || s >= a.path_len[q] || grp < 0 || grp >= g.n_groups) return 0.0;
    if (a.cut_len[q] < s) return 0.0;
    const double d = (double)(s - ti) * a.dl;
    if (d > a.ad.reach) return 0.0;
    int32_t t0 = g.tick[q] - 1;
    if (t0 < 0) t0 += cycle;
    const double kc = ceil(d / (a.ad.v_cruise * a.dt));
    const int32_t k_c = kc < (double)ADVISE_STEPS_MAX ? (int32_t)kc : ADVISE_STEPS_MAX;        // (d > 0 and v_cruise * dt > 0: kc >= 1)
    const int32_t *gr = g.plan_green + 2 * ((size_t)plan * (size_t)g.n_groups + (size_t)grp);
    int64_t u = ((int64_t)t0 + (int64_t)k_c - (int64_t)gr[0]) % (int64_t)cycle;
    if (u < 0) u += cycle;
    if (u < (int64_t)gr[1]) return 0.0;
    const int64_t k_t = (int64_t)k_c + ((int64_t)cycle - u) + (int64_t)a.ad.lead;
    const double v = d / ((double)k_t * a.dt);
    return v > a.ad.v_min ? v : a.ad.v_min;
}

// step 5 for window point t of agent q under the cap v (> 0: advised)
MPCX_REC_FN void advise_clamp(const AdviseArgs &a, int q, int t, double v) {
    double *e = a.xref + ((size_t)4 * (size_t)q + 2) * (size_t)a.W + (size_t)t;
    *e = fmin(*e, v);
}

// the whole rule for agent q on one lane (the host build; the kernel spreads the clamp over a run of lanes); returns advised[q]
MPCX_REC_FN double advise_agent(const AdviseArgs &a, int q) {
    const double v = advise_speed(a, q);
    a.ad.advised[q] = v;
    if (v > 0.0)
        for (int t = 0; t < a.W; t++) advise_clamp(a, q, t, v);
    return v;
}

}  // namespace mpcx
