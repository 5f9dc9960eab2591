// mpcx_intent_core.h -- SHARED PLANS: a connected agent is seen by the others on the plan it solved one step ago, not on its last controls
// held constant.  Host + device source (the pattern of mpcx_advise_core.h).  intent_kernel (mpcx_intent.hip) runs it between the prediction
// and the conflict search of a step; tests/intent_ref/intent_ref.cpp builds it for the host.
//
// The prediction stage (predict_row, mpcx_predict_core.h) is the reference's MovingObstaclesPrediction: the controls applied in the last
// step, held for pred_steps frames.  That is right for a scripted car, which has no plan.  An MPC agent solved a T-step plan one step ago
// and u_sol [P][2][T] (row 0 acceleration, row 1 steering) still holds it when the prediction runs: its braking in front of a cut path, a
// stop line or an advised speed is in there.  The rule re-rolls that plan through the prediction's own model.
//
// For agent q with own pool row r = obs_skip[q], row r's frames are LEFT AS THE PREDICTION STAGE WROTE THEM and frames[q] = 0 if
//   share[q] == 0;  done is given and done[q] != 0;  r outside the pool (refused by the host: never written);  absent is given and
//   absent[r] != 0;  status[q] != MPCX_QP_OPTIMAL (the plant applied max_decel and zeroed the warm start: the constant prediction from
//   `applied` is then the truth).
// Otherwise all pred_steps frames of row r are overwritten and frames[q] = pred_steps:
//   (x, y, v, yaw) = state[q];  frame k = 0 .. pred_steps - 1 takes the planned control j = min(k + 1, T - 1) -- column 0 was applied in
//   the step just taken, beyond the plan the last column is held, which is what the constant prediction does with the one control it knows --
//   acc = u_sol[q][0][j], steer = u_sol[q][1][j], and predict_row's four updates in its order (v BEFORE yaw), v not clamped:
//       x += (v cos yaw) dt;  y += (v sin yaw) dt;  v += acc dt;  yaw += ((v / L) tan steer) dt
//   then the two disc centres of the pose (pose_discs).
// Two consequences are the invariants of the feature, bit for bit on the device: a plan whose columns j >= 1 all equal the applied
// controls leaves predict_kernel's frames, and so does any plan with T = 1.
//
// The text is in parts because the kernel spreads the frames of an agent over the lanes of a group: intent_row is the skip test,
// intent_col the column of a frame, intent_speed / intent_turn / intent_step the updates.  intent_step is `sum + term dt` for x, y and yaw
// alike, in predict_row's spelling: where the device compiler contracts predict_row's product with dt into the sum it does so here (the
// product meets the sum in one block in both kernels), and acc dt -- loop-invariant in predict_row, so rounded on its own -- is rounded on
// its own here too, because it crosses lanes before it is added.  A host build (-ffp-contract=off) rounds every operation.
// Every write is to row obs_skip[q] and frames[q]: the agents' own rows are distinct, so the outcome does not depend on the order of the
// lanes.
#pragma once
#include <math.h>
#include "mpcx_record_core.h"

#if defined(__HIPCC__)
#include "mpcx_predict_core.h"
#define MPCX_INTENT_FN __device__ __forceinline__
#define MPCX_INTENT_ADD(a, b) __dadd_rn(a, b)
#define MPCX_INTENT_MUL(a, b) __dmul_rn(a, b)
#define MPCX_INTENT_DIV(a, b) __ddiv_rn(a, b)
#else       /* g++: every operation is rounded; the host build passes -ffp-contract=off */
#define MPCX_INTENT_FN static inline
#define MPCX_INTENT_ADD(a, b) ((a) + (b))
#define MPCX_INTENT_MUL(a, b) ((a) * (b))
#define MPCX_INTENT_DIV(a, b) ((a) / (b))
#endif

namespace mpcx {

struct IntentArgs {
    mpcx_interaction_params ip;             // pred_steps, dt, L, circle_centers
    int P, T, n_pool;                       // agents; the horizon; rows of the pool
    int has_done, has_absent;               // done / absent are given (tested on the host, as QpArgs::has_warm)
    const double *state;                    // P x 4
    const double *u_sol;                    // P x 2 x T, the previous step's solution
    const int32_t *status;                  // P, of that solution
    const int32_t *obs_skip;                // P, the agents' own pool rows
    const int32_t *done;                    // P or nullptr
    const int32_t *absent;                  // n_pool or nullptr
    double *pred;                           // n_pool x pred_steps x 2 discs x 2, as the prediction stage left it
    mpcx_intent in;
};

// the skip test: agent q's own pool row if its frames are taken from its plan, else -1.  Reads only.
MPCX_INTENT_FN int32_t intent_row(const IntentArgs &a, int q) {
    if (a.in.share[q] == 0) return -1;
    if (a.has_done && a.done[q] != 0) return -1;
    const int32_t r = a.obs_skip[q];
    if (r < 0 || r >= a.n_pool) return -1;
    if (a.has_absent && a.absent[r] != 0) return -1;
    if (a.status[q] != MPCX_QP_OPTIMAL) return -1;
    return r;
}

// the planned control frame k takes
MPCX_INTENT_FN int intent_col(int T, int k) { return k + 1 < T - 1 ? k + 1 : T - 1; }

// v += acc dt, with acc dt rounded on its own (adt)
MPCX_INTENT_FN double intent_impulse(double acc, double dt) { return MPCX_INTENT_MUL(acc, dt); }
MPCX_INTENT_FN double intent_speed(double v, double adt) { return MPCX_INTENT_ADD(v, adt); }
// (v / L) tan steer, v the UPDATED speed, tn = tan(steer)
MPCX_INTENT_FN double intent_turn(double v, double L, double tn) { return MPCX_INTENT_MUL(MPCX_INTENT_DIV(v, L), tn); }
// v cos yaw and v sin yaw of the pose BEFORE the frame
MPCX_INTENT_FN double intent_along(double v, double cs) { return MPCX_INTENT_MUL(v, cs); }
// sum += term dt: x, y and yaw
MPCX_INTENT_FN double intent_step(double sum, double term, double dt) { return MPCX_INTENT_ADD(sum, MPCX_INTENT_MUL(term, dt)); }

#if !defined(__HIPCC__)
// trajectories.py:11-37 (disc_centre / pose_discs of the device code, in their order of operations)
MPCX_INTENT_FN void intent_discs(const mpcx_interaction_params &ip, double px, double py, double c, double s, double *out) {
    for (int d = 0; d < 2; d++) {
        const double cx = ip.circle_centers[2 * d], cy = ip.circle_centers[2 * d + 1];
        out[2 * d] = ((c * cx) + -(s * cy)) + px;
        out[2 * d + 1] = ((s * cx) + (c * cy)) + py;
    }
}

// the whole rule for agent q on one lane (the host build; the kernel spreads the frames over a group of lanes); returns frames[q]
MPCX_INTENT_FN int32_t intent_agent(const IntentArgs &a, int q) {
    const int32_t r = intent_row(a, q);
    if (r < 0) { a.in.frames[q] = 0; return 0; }
    const double *st = a.state + 4 * (size_t)q, *u = a.u_sol + 2 * (size_t)a.T * (size_t)q;
    const double dt = a.ip.dt;
    double x = st[0], y = st[1], v = st[2], yaw = st[3], sn, cs;
    double *out = a.pred + (size_t)r * (size_t)a.ip.pred_steps * 4;
    sincos(yaw, &sn, &cs);          // one sincos per pose, as the kernel takes it
    for (int k = 0; k < a.ip.pred_steps; k++) {
        const int j = intent_col(a.T, k);
        const double acc = u[j], tn = tan(u[a.T + j]);
        x = intent_step(x, intent_along(v, cs), dt);
        y = intent_step(y, intent_along(v, sn), dt);
        v = intent_speed(v, intent_impulse(acc, dt));
        yaw = intent_step(yaw, intent_turn(v, a.ip.L, tn), dt);
        sincos(yaw, &sn, &cs);
        intent_discs(a.ip, x, y, cs, sn, out + 4 * k);
    }
    a.in.frames[q] = a.ip.pred_steps;
    return a.ip.pred_steps;
}
#endif

}  // namespace mpcx
