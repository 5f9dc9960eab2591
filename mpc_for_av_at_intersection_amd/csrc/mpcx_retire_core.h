// mpcx_retire_core.h -- retirement at the goal for ONE agent and step, host + device source (the pattern of mpcx_record_core.h and
// mpcx_traffic_core.h).  retire_kernel (mpcx_retire.hip) runs it one lane per agent as the LAST launch of a closed-loop step, after the
// record stage (so the final log row holds the controls really applied); tests/retire_ref/retire_ref.cpp builds it for the host.
//
// The end of the reference's loop is `if mpc.is_goal(state): break` at the top of an iteration (scenarios/mpc_intersection.py:92-93).
// After step s that is the test on the state the plant step of s left, with this step's target_ind and len(self.cx) -- exactly what the
// run log evaluates for goal_step, so the test itself is rec_is_goal of mpcx_record_core.h, called here, not restated:
//   len(self.cx)   goal_len[q]: the loop passes cut_len in cut mode and path_len in speed mode (the whole path; cut_len holds the stop
//                  index there)
//   goal           the LAST point of the agent's full path
// For an agent that is still driving (done[q] == 0) the rule counts the step in steps_driven[q] and, where the test holds, sets
// done[q] = 1 and zeroes applied[q]: to the other agents a retired car is parked, without acceleration or steering (the last real controls
// of a decelerating ego would make the prediction roll it backwards over the whole horizon).  A retired agent's words are left alone.
// With a scene (mpcx_scene: departure) the arrival also sets absent[own_row[q]], the word of the agent's own pool row (the loop passes obs_skip,
// which names that row with and without scripted traffic): from the next step on the car is gone from everybody's obstacle list.  Agents'
// rows are distinct rows, so this too is a word no other lane touches; a row outside the pool is never written.
// Per agent it reads 3 + 3 doubles and four words and writes at most three words and two doubles; no lane reads what another lane writes.
#pragma once
#include "mpcx_record_core.h"

namespace mpcx {

struct RetireArgs {
    int P;
    const double *state, *path_xyyaw;
    double *applied;
    const int32_t *path_off, *path_len, *target_ind, *goal_len;
    mpcx_retire r;
    int32_t *absent = nullptr;              // departure (mpcx_scene::absent, n_rows words) or nullptr: none
    const int32_t *own_row = nullptr;       // ... the agent's own pool row (obs_skip)
    int32_t n_rows = 0;
};

// returns whether the agent arrived in this step
MPCX_REC_FN bool retire_agent(const RetireArgs &a, int q) {
    if (a.r.done[q] != 0) return false;
    a.r.steps_driven[q] += 1;
    const int32_t len = a.path_len[q];
    if (len <= 0) return false;
    const double *st = a.state + 4 * (size_t)q;
    const double *g = a.path_xyyaw + 3 * ((size_t)a.path_off[q] + len - 1);
    if (!rec_is_goal(st[0], st[1], st[2], g[0], g[1], a.target_ind[q], a.goal_len[q], a.r.goal_dis, a.r.stop_speed)) return false;
    a.r.done[q] = 1;
    a.applied[2 * (size_t)q] = 0.0; a.applied[2 * (size_t)q + 1] = 0.0;
    if (a.absent) {
        const int32_t row = a.own_row[q];
        if (row >= 0 && row < a.n_rows) a.absent[row] = 1;
    }
    return true;
}

}  // namespace mpcx
