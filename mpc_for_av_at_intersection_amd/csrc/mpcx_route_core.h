// mpcx_route_core.h -- ROUTES: every vehicle of a respawning slot takes its own route from its own start pose.  Host + device source (the
// pattern of mpcx_respawn_core.h).  respawn_route_kernel (mpcx_route.hip) runs it one lane per agent IN PLACE OF respawn_kernel;
// tests/route_ref/route_ref.cpp builds it for the host.
//
// Vehicle g of slot q drives route route_of[q][g] -- an index into route_off / route_len (R words each), which name runs of the path tables:
// path_off[q] and path_len[q] are caller-owned device words that every stage reads afresh in every step, and every path table is indexed by
// absolute path point, so a vehicle's route is two more words for the reset to write -- from start_state[q][g] and index start_idx[q][g].
// For agent q, in this order:
//   1. g = served[q], read before anything else
//   2. respawn_agent (mpcx_respawn_core.h): the episode record, served[q] += 1 and, with vehicles left, the reset and the hand-over to the gate
//   3. if it returned true (the agent arrived): ep_i32[q][g][7] = route_of[q][g], the episode's route in the record's reserved word
//   4. if the slot was reset (served[q] < G now), with g' = g + 1 and r = route_of[q][g'], what the reset just wrote is overwritten:
//        state[q] = start_state[q][g'], traj_idx[q] = target_ind[q] = start_idx[q][g'], path_off[q] = route_off[r], path_len[q] = route_len[r]
//   5. a DEFECTIVE next vehicle -- r outside [0, R), or start_idx[q][g'] outside [0, route_len[r]) -- is never driven: the slot is left with
//      wait = -1, entered_step = -1, done set and its row absent (as retirement and departure left them).  It then neither drives nor
//      waits, and respawn's own precondition (entered_step >= 0) never holds for it again.  path_off and path_len are not touched.
// Every access is to words of agent q (its own records and rows of the per-vehicle tables included) plus the read-only route tables, so no
// lane reads what another lane of the launch writes and the outcome does not depend on the order of the lanes.  A driving agent costs one
// load.  The last vehicle of a slot writes its record and nothing else: path_off and path_len stay its own.
#pragma once
#include "mpcx_respawn_core.h"

namespace mpcx {

struct RouteArgs {
    RespawnArgs r;
    mpcx_routes rt;
};

// returns whether the agent arrived (an episode record was written)
MPCX_REC_FN bool route_agent(const RouteArgs &a, int q) {
    const int32_t g = a.r.rs.served[q];
    if (!respawn_agent(a.r, q)) return false;
    const int32_t G = a.r.rs.generations;
    const size_t e = (size_t)q * (size_t)G + (size_t)g;
    a.r.rs.ep_i32[RESPAWN_I32 * e + 7] = a.rt.route_of[e];
    if (g + 1 >= G) return true;            // the last vehicle: no reset
    const int32_t r = a.rt.route_of[e + 1], s0 = a.rt.start_idx[e + 1];
    const int32_t len = (r >= 0 && r < a.rt.n_routes) ? a.rt.route_len[r] : 0;
    if (len <= 0 || s0 < 0 || s0 >= len) {  // defective: never driven
        a.r.ad.wait[q] = -1;
        a.r.ad.entered_step[q] = -1;
        return true;
    }
    for (int k = 0; k < 4; k++) a.r.state[4 * (size_t)q + k] = a.rt.start_state[4 * (e + 1) + k];
    a.r.traj_idx[q] = s0; a.r.target_ind[q] = s0;
    a.rt.path_off[q] = a.rt.route_off[r];
    a.rt.path_len[q] = a.rt.route_len[r];
    return true;
}

// ---- the per-movement summary of a routed run (mpcx_episode_summary): the definition, one record at a time.  acc = (count, contacts,
// sum of entered - due, sum of steps_driven); integer sums and a minimum only, so the table is exact in any order.
MPCX_REC_FN void summary_take(const int32_t *w /*8*/, const double *f /*2*/, int64_t (&acc)[4], double &lo) {
    acc[0] += 1;
    acc[1] += w[4] >= 0 ? 1 : 0;
    acc[2] += (int64_t)w[0] - (int64_t)w[6];
    acc[3] += (int64_t)w[2];
    lo = f[0] < lo ? f[0] : lo;             // (a NaN is skipped)
}

}  // namespace mpcx
