// mpcx_record_core.h -- the run log's record rule for ONE agent and step, host + device source (the pattern of mpcx_traffic_core.h).
// record_kernel (mpcx_record.hip) runs it one lane per agent as the last launch of a closed-loop step; tests/record_ref/record_ref.cpp
// builds it for the host.  It is evaluated AFTER the plant step of step s on the buffers the loop holds anyway:
//
//   row (8 doubles)  x, y, v, yaw     state[q] after the plant step (History's convention: stored after simulation.step,
//                                      main/lib/simulation.py:58-88)
//                    accel, steer     applied[q] of this step (applied is (steer, accel); after a failed solve what the plant really applied)
//                    xref_deviation   main/lib/mpc.py:301-308 verbatim, component-wise:
//                                        hypot(cos(cyaw[t] + pi/2) * (cx[t] - ox0), sin(cyaw[t] + pi/2) * (cy[t] - oy0)),   t = target_ind[q],
//                                      (ox0, oy0) = x_sol[q][0..1][0], the state BEFORE the step; NaN after a failed solve (the reference's
//                                      ox is None there; NaN is History.store's "no value")
//                    clearance        true distance at the START of the step: over every pool row r of the agent's window
//                                      [obs_off, obs_off + obs_cnt) except its own row obs_skip[q], and every pair of discs,
//                                      min |c_ego - c_r| - 2 radius.  Poses from the pool as this step's conflict search saw them (the pool
//                                      is written at the start of a step and not touched again); the ego's own pose is its own pool row.
//                                      +inf if the window holds nobody else (or the agent has no row of its own to compare from).
//                                      With a scene (mpcx_scene) the rows with absent[r] != 0 are left out, as the step's conflict search left
//                                      them out; the agent's own row is its pose whether it is absent (a ghost) or not.
//   row (8 int32)    traj_idx, target_ind, cut_len, hit_idx, status, iters as they stand after the step, 0, 0
//
// and the per-agent outcome words, which exist whatever the row capacity:
//   steps          rows offered so far = the agent's write cursor.  Device memory, one word per agent: the launch carries no step index
//                  (a replayed hipGraph keeps advancing), and no lane reads a word another lane writes.
//   goal_step      steps taken when mpc.is_goal (main/lib/mpc.py:310-326) first held, else -1: goal = the LAST point of the agent's full
//                  path, len(self.cx) = this step's cut_len (goal_len[q] where goal_len is given: the speed-reference loop of
//                  main/scenarios/mpc_intersection_new_ref.py keeps the whole path, len(self.cx) = path_len, and the cut_len column holds
//                  its stop index), self.target_ind = this step's target_ind, state after the plant step.  After
//                  step s that is the reference's test at the top of iteration s + 1, so goal_step is the reference's number of loop
//                  iterations.  Set once.
//   flags, contact_step, min_clearance   AFTER SEPARATION: flags bit 0 = "has been clear" (a step with clearance >= 0 was seen);
//                  min_clearance = minimum of clearance from that step on (+inf before), contact_step = first step with clearance < 0
//                  after it, else -1.  (The reference's stock scenario spawns its second scripted car ON the ego's start pose: a plain
//                  first contact would be step 0 there.  The rows keep the raw value.)
// The window is walked over at most MPCX_MAX_OBS + 1 rows (what the conflict search handles; it flags a larger one with hit_idx -2), every
// pool index is checked against the pool before it is read.
// Under retirement at the goal (mpcx_retire) the rule is not run for a retired agent: its cursor stops at goal_step, its outcome words
// stay, and the goal test below is the one mpcx_retire_core.h calls for the retirement itself.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mpcx.h"

#if defined(__HIPCC__)
#define MPCX_REC_FN __host__ __device__ __forceinline__
#else
#define MPCX_REC_FN static inline
#endif

namespace mpcx {

constexpr double REC_PI = 3.141592653589793;      // numpy.pi
constexpr int REC_F64 = 8, REC_I32 = 8;           // columns of a row

struct RecordArgs {
    int P, n_pool;
    int64_t x_stride;               // doubles between the solutions of two agents: 4 (T + 1)
    double radius, cc[4];           // mpcx_interaction_params.radius / circle_centers
    const double *state, *applied, *x_sol, *path_xyyaw, *obs6;
    const int32_t *path_off, *path_len, *target_ind, *cut_len, *traj_idx, *hit_idx, *status, *iters;
    const int32_t *obs_off, *obs_cnt, *obs_skip;
    mpcx_run_log log;
    const int32_t *goal_len = nullptr;      // len(self.cx) of the goal test per agent; nullptr: cut_len
    const int32_t *done = nullptr;          // retirement (mpcx_retire::done) or nullptr: record_kernel skips an agent with done[q] != 0 entirely
    const int32_t *absent = nullptr;        // departure (mpcx_scene::absent, n_pool words) or nullptr: the clearance skips pool rows with absent[r] != 0
};

MPCX_REC_FN void rec_sincos(double a, double *s, double *c) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(a, s, c);
#else
    *s = sin(a); *c = cos(a);
#endif
}

// (x, y) of the two discs of a car at pose (x, y, yaw): trajectories.py:11-37
MPCX_REC_FN void rec_discs(const double *cc, double x, double y, double yaw, double *d4) {
    double s, c;
    rec_sincos(yaw, &s, &c);
    d4[0] = x + (c * cc[0] - s * cc[1]); d4[1] = y + (s * cc[0] + c * cc[1]);
    d4[2] = x + (c * cc[2] - s * cc[3]); d4[3] = y + (s * cc[2] + c * cc[3]);
}

MPCX_REC_FN double rec_clearance(const RecordArgs &a, int q) {
    const int own = a.obs_skip[q];
    if (own < 0 || own >= a.n_pool) return INFINITY;
    const double *e = a.obs6 + 6 * (size_t)own;
    double ed[4];
    rec_discs(a.cc, e[0], e[1], e[3], ed);
    const int off = a.obs_off[q];
    int cnt = a.obs_cnt[q];
    if (cnt > MPCX_MAX_OBS + 1) cnt = MPCX_MAX_OBS + 1;
    double best = INFINITY;
    for (int k = 0; k < cnt; k++) {
        const int r = off + k;
        if (r == own || r < 0 || r >= a.n_pool) continue;
        if (a.absent && a.absent[r] != 0) continue;         // departed (or hidden): not in the scene
        const double *o = a.obs6 + 6 * (size_t)r;
        double od[4];
        rec_discs(a.cc, o[0], o[1], o[3], od);
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 2; j++)
                best = fmin(best, hypot(ed[2 * i] - od[2 * j], ed[2 * i + 1] - od[2 * j + 1]));
    }
    return best - 2.0 * a.radius;
}

// mpc.py:301-308; pt = (cx, cy, cyaw) of the target point
MPCX_REC_FN double rec_deviation(const double *pt, double ox0, double oy0) {
    double s, c;
    rec_sincos(pt[2] + REC_PI / 2, &s, &c);
    return hypot(c * (pt[0] - ox0), s * (pt[1] - oy0));
}

// mpc.py:310-326
MPCX_REC_FN bool rec_is_goal(double x, double y, double v, double gx, double gy, int target_ind, int cut_len, double goal_dis, double stop_speed) {
    int gap = target_ind - cut_len;
    if (gap < 0) gap = -gap;
    return hypot(x - gx, y - gy) <= goal_dis && gap < 5 && fabs(v) <= stop_speed;
}

// the "after separation" outcome of step s with clearance c
MPCX_REC_FN void rec_outcome(double c, int32_t s, int32_t *flags, int32_t *contact_step, double *min_clearance) {
    if (c >= 0.0) *flags |= 1;
    if (*flags & 1) {
        *min_clearance = fmin(*min_clearance, c);
        if (c < 0.0 && *contact_step < 0) *contact_step = s;
    }
}

// The whole rule for agent q: fills the row, updates the agent's outcome words and its cursor, returns the cursor as it was (= the
// 0-based index of the step; the row belongs into rows[s] if s < capacity).
MPCX_REC_FN int32_t record_agent(const RecordArgs &a, int q, double *f, int32_t *w) {
    const double *st = a.state + 4 * (size_t)q;
    const int32_t target = a.target_ind[q], cut = a.cut_len[q], status = a.status[q];
    const int32_t off = a.path_off[q], len = a.path_len[q];
    f[0] = st[0]; f[1] = st[1]; f[2] = st[2]; f[3] = st[3];
    f[4] = a.applied[2 * (size_t)q + 1];
    f[5] = a.applied[2 * (size_t)q];
    double dev = NAN;
    if (status == 0 && target >= 0 && target < len) {
        const double *xs = a.x_sol + (size_t)a.x_stride * q;
        dev = rec_deviation(a.path_xyyaw + 3 * ((size_t)off + target), xs[0], xs[a.x_stride / 4]);
    }
    f[6] = dev;
    const double c = rec_clearance(a, q);
    f[7] = c;
    w[0] = a.traj_idx[q]; w[1] = target; w[2] = cut; w[3] = a.hit_idx[q]; w[4] = status; w[5] = a.iters[q];
    w[6] = 0; w[7] = 0;
    const int32_t s = a.log.steps[q];
    if (a.log.goal_step[q] < 0 && len > 0) {
        const double *g = a.path_xyyaw + 3 * ((size_t)off + len - 1);
        if (rec_is_goal(st[0], st[1], st[2], g[0], g[1], target, a.goal_len ? a.goal_len[q] : cut, a.log.goal_dis, a.log.stop_speed)) a.log.goal_step[q] = s + 1;
    }
    int32_t flags = a.log.flags[q], contact = a.log.contact_step[q];
    double minc = a.log.min_clearance[q];
    rec_outcome(c, s, &flags, &contact, &minc);
    a.log.flags[q] = flags; a.log.contact_step[q] = contact; a.log.min_clearance[q] = minc;
    a.log.steps[q] = s + 1;
    return s;
}

}  // namespace mpcx
