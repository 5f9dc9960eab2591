// mpcx_brake_core.h -- FIRM HOLD: in speed mode an agent that a hold keeps at its stop line really stops in front of it.  Host + device
// source (the pattern of mpcx_follow_core.h).  brake_mark_kernel (mpcx_brake.hip) runs it behind the last hold stage and the following
// stage of a closed-loop step, in front of the window stage; brake_clamp_kernel behind every window stage, beside the advice and following
// clamps; tests/brake_ref/brake_ref.cpp builds it for the host.
//
// Every rule that stops a car at a line -- signals, actuated signals, reservations, keep clear, the priority road, stop signs -- lowers cut_len to the
// line's index s.  In cut mode the path ends there.  In speed mode the path stays whole and only the speed reference is zeroed from s on,
// and that does not hold a car, for two reasons: (1) the window advances by cumsum(max(v, 10 / 3.6) dt), so the POSITION reference of a
// standing car runs ahead at 2.78 m/s, over the line; (2) calc_nearest_index_in_direction(forward) answers start + 1 for a car that stands
// on `start`, so traj_idx climbs a point a step and a car that stands 2 m before its line is "on or past the line", and free, after
// s - traj_idx steps.  The rule ends the position reference on a stop point in front of the line, puts a braking profile on the speed
// reference and pins the index while the car is physically behind the line.
//
// Agent q is LINE-HELD in a step if done[q] == 0, one of the hold words that are on in that step is nonzero for it (held, boxed, yielding --
// under stop signs the loop hands the stage's stopping in yielding's place --: a null pointer is a word that is off), and s = path_stop[path_off[q] + traj_idx[q]] is a valid line ahead by the hold's own test
// (signal_hold): i = path_off[q] + traj_idx[q] in [0, n_points), 0 <= traj_idx[q] < s < path_len[q]; and path_off[q] + s lies in the table
// too.  Then m = ceil(setback / dl), e = max(s - m, 2) -- the length of the path as the window is to see it --, E = path point e - 1.
//   MARK (one lane per agent, in front of the window stage): firm[q] = e for a line-held agent, else 0; brake_cap[q] = 0.0.  In speed mode
//      win_len[q] = e and target_ind[q] = min(target_ind[q], e - 1) for a line-held agent and win_len[q] = path_len[q] for everybody else:
//      the window stage is handed win_len in place of path_len, so it builds a line-held agent's window on full[:e] and every other
//      agent's exactly as it did.  In cut mode nothing else is written: the cut is hard already.
//   CLAMP (speed mode, behind every window stage), for an agent with firm[q] = e != 0 whose line still checks out:
//      b. every entry t of row 2 of q's xref becomes fmin(entry, sqrt(2 brake d_t)), d_t = the Euclidean distance of window point t (rows 0
//         and 1 of xref) to E: 0 at E, and a zero stays a zero.
//      c. q is BEHIND ITS LINE iff (x - p_s.x)(p_s.x - p_{s-1}.x) + (y - p_s.y)(p_s.y - p_{s-1}.y) < 0, p_s the line's path point: a half-plane
//         through the line, no trigonometry.  Behind: traj_idx[q] = min(traj_idx[q], e - 1) -- the holds have read traj_idx by now.  Not
//         behind, a physical overrun: nothing is pinned, the hold's "on or past the line" frees the agent as ever, overran[q] += 1.
//      d. brake_cap[q] = the profile at window point 0; len_seen[q] = path_len[q], which the window stage left at e: the next conflict
//         search's prev_cut_len stays the whole path's.
// Every product and sum is a statement of its own under "contract off" (host builds pass -ffp-contract=off); sqrt, ceil and the division
// are correctly rounded: host and device agree bit for bit.  No sin / cos.  Every write is to words of agent q, and nothing a lane reads is
// written by another lane, so the outcome does not depend on the order of the lanes; everything mutable is device memory: a replayed
// hipGraph behaves like a plain run.
#pragma once
#include <math.h>
#include "mpcx_record_core.h"

#if defined(__clang__)
#define MPCX_BRAKE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else       /* g++ honours no such pragma: a host build with it passes -ffp-contract=off */
#define MPCX_BRAKE_NO_CONTRACT
#endif

namespace mpcx {

constexpr int32_t BRAKE_STEPS_MAX = 1 << 30;        // the clamp of the setback in points

struct BrakeArgs {
    int P, W;                               // agents; window points T + 1 (the clamp)
    int speed;                              // the stop mode is MPCX_STOP_SPEED
    double dl;
    const double *state;                    // P x 4 (the clamp)
    const double *path_xyyaw;               // the path tables, 3 doubles a point (the clamp)
    const int32_t *path_off, *path_len;     // P each
    int32_t *traj_idx;                      // P, as the holds read it; the clamp pins it
    int32_t *target_ind;                    // P, in-out (the mark, speed mode)
    int32_t *win_len;                       // P, out (the mark, speed mode): the length the window stage is to use
    int32_t *len_seen;                      // P or nullptr (the clamp): restored to path_len for a line-held agent
    const int32_t *done;                    // P or nullptr
    const int32_t *path_stop;               // n_points: route-local index of the next stop line at or after the point, -1 = none
    int32_t n_points;
    const int32_t *held, *boxed, *yielding; // P each or nullptr: the hold words that are on in this step
    double *xref;                           // P x 4 x W (the clamp)
    mpcx_braking br;
};

// the line ahead of agent q by the hold's own test, and the stop index: s, e; false: no valid line ahead
MPCX_REC_FN bool brake_line(const BrakeArgs &a, int q, int32_t *s_out, int32_t *e_out) {
    MPCX_BRAKE_NO_CONTRACT
    const int32_t ti = a.traj_idx[q];
    const int64_t off = a.path_off[q];
    const int64_t i = off + (int64_t)ti;
    if (ti < 0 || i < 0 || i >= (int64_t)a.n_points) return false;
    const int32_t s = a.path_stop[i];
    if (!(s >= 0 && ti < s && s < a.path_len[q])) return false;
    if (off < 0 || off + (int64_t)s >= (int64_t)a.n_points) return false;
    const double md = ceil(a.br.setback / a.dl);
    const int32_t m = md < (double)BRAKE_STEPS_MAX ? (int32_t)md : BRAKE_STEPS_MAX;           // (NaN: the clamp)
    const int64_t e = (int64_t)s - (int64_t)m;
    *s_out = s;
    *e_out = e > 2 ? (int32_t)e : 2;
    return true;
}

// one of the hold words that are on is nonzero for agent q
MPCX_REC_FN bool brake_word(const BrakeArgs &a, int q) {
    return (a.held && a.held[q] != 0) || (a.boxed && a.boxed[q] != 0) || (a.yielding && a.yielding[q] != 0);
}

// MARK for agent q on one lane; returns firm[q]
MPCX_REC_FN int32_t brake_mark_agent(const BrakeArgs &a, int q) {
    int32_t s = 0, e = 0;
    const bool on = !(a.done && a.done[q] != 0) && brake_word(a, q) && brake_line(a, q, &s, &e);
    a.br.firm[q] = on ? e : 0;
    a.br.brake_cap[q] = 0.0;
    if (a.speed) {
        a.win_len[q] = on ? e : a.path_len[q];
        if (on && a.target_ind[q] > e - 1) a.target_ind[q] = e - 1;
    }
    return on ? e : 0;
}

// what the clamp needs of a line-held agent: the stop point and the line's half-plane
struct BrakeLine {
    int32_t s, e;
    double ex, ey;                          // E
    double sx, sy, nx, ny;                  // p_s and p_s - p_{s-1}
};

// the clamp's own look at agent q: firm[q] != 0 and the line it was marked for still checks out (a stage call may be handed any words)
MPCX_REC_FN bool brake_clamp_line(const BrakeArgs &a, int q, BrakeLine *l) {
    MPCX_BRAKE_NO_CONTRACT
    if (a.done && a.done[q] != 0) return false;
    const int32_t e = a.br.firm[q];
    if (e == 0) return false;
    int32_t s = 0, e2 = 0;
    if (!brake_line(a, q, &s, &e2) || e2 != e) return false;
    const double *path = a.path_xyyaw + 3 * (size_t)a.path_off[q];
    l->s = s; l->e = e;
    l->ex = path[3 * (size_t)(e - 1)]; l->ey = path[3 * (size_t)(e - 1) + 1];
    l->sx = path[3 * (size_t)s]; l->sy = path[3 * (size_t)s + 1];
    l->nx = l->sx - path[3 * (size_t)(s - 1)];
    l->ny = l->sy - path[3 * (size_t)(s - 1) + 1];
    return true;
}

// b. the profile's value at a window point (px, py)
MPCX_REC_FN double brake_profile(double brake, double px, double py, double ex, double ey) {
    MPCX_BRAKE_NO_CONTRACT
    const double dx = px - ex, dy = py - ey;
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double d2 = xx + yy;
    const double d = sqrt(d2);
    const double b2 = 2.0 * brake;
    const double bd = b2 * d;
    return sqrt(bd);
}

// b. for window point t of agent q
MPCX_REC_FN void brake_clamp_point(const BrakeArgs &a, int q, int t, double ex, double ey) {
    double *x = a.xref + (size_t)4 * (size_t)q * (size_t)a.W + (size_t)t;
    double *v = x + 2 * (size_t)a.W;
    *v = fmin(*v, brake_profile(a.br.brake, x[0], x[a.W], ex, ey));
}

// c. and d. for agent q with its line l, once per clamp
MPCX_REC_FN void brake_clamp_words(const BrakeArgs &a, int q, const BrakeLine &l) {
    MPCX_BRAKE_NO_CONTRACT
    const double *x0 = a.xref + (size_t)4 * (size_t)q * (size_t)a.W;
    a.br.brake_cap[q] = brake_profile(a.br.brake, x0[0], x0[a.W], l.ex, l.ey);
    const double rx = a.state[4 * (size_t)q] - l.sx, ry = a.state[4 * (size_t)q + 1] - l.sy;
    const double ax = rx * l.nx;
    const double ay = ry * l.ny;
    const double side = ax + ay;
    if (side < 0.0) {
        if (a.traj_idx[q] > l.e - 1) a.traj_idx[q] = l.e - 1;
    } else {
        a.br.overran[q] = a.br.overran[q] + 1;
    }
    if (a.len_seen) a.len_seen[q] = a.path_len[q];
}

// CLAMP for agent q on one lane (the host build; the kernel spreads the window points over lanes)
MPCX_REC_FN void brake_clamp_agent(const BrakeArgs &a, int q) {
    BrakeLine l;
    if (!brake_clamp_line(a, q, &l)) return;
    brake_clamp_words(a, q, l);             // (reads window point 0's position, which the profile does not change)
    for (int t = 0; t < a.W; t++) brake_clamp_point(a, q, t, l.ex, l.ey);
}

}  // namespace mpcx
