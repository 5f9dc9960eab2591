// mpcx_respawn_core.h -- RESPAWN: a departed agent's slot is re-used for the next vehicle of its stream.  Host + device source (the pattern of
// mpcx_retire_core.h and mpcx_admit_core.h).  respawn_kernel (mpcx_respawn.hip) runs it one lane per agent as the LAST launch of a
// closed-loop step, after retire_kernel; tests/respawn_ref/respawn_ref.cpp builds it for the host.
//
// A slot (agent index q) serves G = generations vehicles one after the other, all on the slot's route from the slot's start pose
// (start_state[q], start_idx[q]).  served[q] counts the episodes finished so far.  `clock` is admission's word as THIS step's admission stage
// left it: already advanced, so it is the index of the NEXT step and this step is clock - 1.
// Agent q HAS ARRIVED iff done[q] != 0 (retired), wait[q] == -1 (not waiting to enter), entered_step[q] >= 0 (it has been in the scene),
// served[q] < G (the slot is not finished) and its own row own_row[q] lies inside the pool.  On arrival, in this order:
//   1. episode record g = served[q] of slot q:
//        ep_i32[q][g][0..7] = entered_step, arrived_step = clock - 1, steps_driven, row_end = the run log's cursor steps[q] (-1 without a
//                             log), the log's contact_step (in cursor units; -1 if none or no log), the log's flags (0 without), due[q][g], 0
//        ep_f64[q][g][0..1] = the log's min_clearance (+inf without a log), 0
//      The episode's rows of the run log are [row_end - steps_driven, row_end) of the slot's rows.
//   2. served[q] += 1
//   3. if served[q] < G the slot is RESET to "first step of a fresh batch" and handed to the admission gate:
//        state = start_state, applied = 0, traj_idx = target_ind = start_idx, cut_len = 0 (MPCX_STOP_SPEED: prev_len = 0 too), u_sol = 0 (all
//        2 T doubles), iters = 0, steps_driven = 0; with a log goal_step = contact_step = -1, flags = 0, min_clearance = +inf -- the cursor
//        steps[q] is NOT reset: a slot's log rows are its vehicles' rows one after the other;
//        entered_step = -1 and wait = max(0, due[q][served[q]] - clock): the next vehicle asks to enter in step max(next step, its due step)
//        and goes through the gate like any scheduled agent.  done[q] and absent[own row] stay set, as retirement and departure left them:
//        a reset slot is a WAITING agent in exactly the state admission defines.
//   4. otherwise (served[q] == G) the slot is finished: it stays departed and is never touched again.
// Those are all the words a first step READS.  The pure outputs -- x_sol, xref, xbar, reaches_end, status, kkt, hit_idx, hit_xy -- stay as the
// last vehicle left them until the new vehicle's first step overwrites them; nothing reads them for a waiting agent.
// steps_driven == arrived_step - entered_step + 1 for every record, because an agent in the scene drives every step.  The exception is a
// slot found arrived when respawn is switched on (done, not waiting, entered_step >= 0 -- an agent that arrived before, or one retired by the
// host's goal test before the first step, if it was not scheduled): it counts as arriving in that step, with whatever steps_driven holds.
// Every access is to words of agent q only (its own records included), so no lane reads what another lane of the launch writes and the
// outcome does not depend on the order of the lanes.  A driving agent costs one load.
#pragma once
#include "mpcx_record_core.h"

namespace mpcx {

constexpr int RESPAWN_I32 = 8, RESPAWN_F64 = 2;     // words of an episode record

struct RespawnArgs {
    int P, n_pool, u_len;           // u_len: doubles of u_sol per agent, 2 T
    int has_log, has_prev_len;      // tested on the host (as QpArgs::has_warm is)
    double *state, *applied, *u_sol;
    int32_t *traj_idx, *target_ind, *cut_len, *iters, *prev_len;
    const int32_t *own_row;         // obs_skip
    const int32_t *done;            // mpcx_retire::done
    int32_t *steps_driven;          // mpcx_retire::steps_driven
    mpcx_admit ad;
    mpcx_run_log log;               // has_log
    mpcx_respawn rs;
};

// returns whether the agent arrived (an episode record was written)
MPCX_REC_FN bool respawn_agent(const RespawnArgs &a, int q) {
    if (a.done[q] == 0) return false;
    if (a.ad.wait[q] != -1) return false;
    const int32_t entered = a.ad.entered_step[q];
    if (entered < 0) return false;
    const int32_t G = a.rs.generations, g = a.rs.served[q];
    if (g < 0 || g >= G) return false;
    const int32_t own = a.own_row[q];
    if (own < 0 || own >= a.n_pool) return false;
    const int32_t clock = *a.ad.clock;
    const size_t e = (size_t)q * (size_t)G + (size_t)g;
    int32_t *w = a.rs.ep_i32 + RESPAWN_I32 * e;
    double *f = a.rs.ep_f64 + RESPAWN_F64 * e;
    w[0] = entered;
    w[1] = clock - 1;
    w[2] = a.steps_driven[q];
    w[3] = a.has_log ? a.log.steps[q] : -1;
    w[4] = a.has_log ? a.log.contact_step[q] : -1;
    w[5] = a.has_log ? a.log.flags[q] : 0;
    w[6] = a.rs.due[e];
    w[7] = 0;
    f[0] = a.has_log ? a.log.min_clearance[q] : (double)INFINITY;
    f[1] = 0.0;
    a.rs.served[q] = g + 1;
    if (g + 1 >= G) return true;
    for (int k = 0; k < 4; k++) a.state[4 * (size_t)q + k] = a.rs.start_state[4 * (size_t)q + k];
    a.applied[2 * (size_t)q] = 0.0; a.applied[2 * (size_t)q + 1] = 0.0;
    const int32_t s0 = a.rs.start_idx[q];
    a.traj_idx[q] = s0; a.target_ind[q] = s0;
    a.cut_len[q] = 0;
    if (a.has_prev_len) a.prev_len[q] = 0;
    double *u = a.u_sol + (size_t)a.u_len * q;
    for (int k = 0; k < a.u_len; k++) u[k] = 0.0;
    a.iters[q] = 0;
    a.steps_driven[q] = 0;
    if (a.has_log) {
        a.log.goal_step[q] = -1; a.log.contact_step[q] = -1; a.log.flags[q] = 0;
        a.log.min_clearance[q] = (double)INFINITY;
    }
    a.ad.entered_step[q] = -1;
    const int32_t left = a.rs.due[e + 1] - clock;
    a.ad.wait[q] = left > 0 ? left : 0;
    return true;
}

}  // namespace mpcx
