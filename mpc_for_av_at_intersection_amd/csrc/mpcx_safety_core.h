// mpcx_safety_core.h -- the NEAR-MISS LOG: who came close to whom, how close, and how many frames from a predicted contact.  Host + device
// source (the pattern of mpcx_follow_core.h).  safety_kernel (mpcx_safety.hip) runs it directly behind the conflict search of a closed-loop
// step, safety_summary_kernel reduces its events to a conflict matrix; tests/safety_ref/safety_ref.cpp builds both for the host.
//
// The stage decides nothing: it reads obs6 (the pool as the head of this step packed it), the prediction of every pool row as the conflict
// search read it (pred, [row][frame][2 discs][2], after the intent stage), traj_idx as the conflict search left it, path_off, state, done and
// absent, and writes only words of its own, all of them words of agent q.
//
// For agent q with own row o = obs_skip[q]:
//   THE OTHERS: following's -- the rows of its pool window [obs_off[q], obs_off[q] + obs_cnt[q]) other than o, in row order, the first
//      MPCX_MAX_OBS of them (slot j <-> pool row safety_slot_row()); a row outside the pool or with absent[r] != 0 is left out.  Precedence
//      words are not consulted: a yielding car is measured on its real prediction.
//   NOT MEASURED: done[q] != 0, o outside the pool, absent[o] != 0, no others.  Every per-step word is "none", the open encounter is closed,
//      the tick advances all the same.
//   1. NOW.  c_now = min over the others and the 2 x 2 pairs of discs of hypot(..) - 2 radius at the poses of obs6 (rec_discs of
//      mpcx_record_core.h: on the device the run log's clearance of the step, bit for bit); r_now = its row, the lowest slot of equals.
//      Nobody: +inf, -1.
//   2. PREDICTED CONTACT.  d2(r, k) = min over the 2 x 2 pairs of dx dx + dy dy between pred[o][k] and pred[r][k]; k(r) = the lowest k in
//      [0, pred_steps) with d2(r, k) < (2 radius)^2; (k_ttc, r_ttc) = the smallest k(r), the lowest slot of equals (key k << 8 | slot).
//      None: -1, -1.  Frame k is the pose (k + 1) dt ahead.
//   3. WORDS of the step: partner = r_now, clearance = c_now, ttc_row = r_ttc, ttc_frame = k_ttc.
//   4. ENCOUNTERS.  critical = c_now < near or 0 <= k_ttc < ttc_frames; its partner p = r_now if c_now < near, else r_ttc.  enc_row[q] is the
//      partner of the open encounter (-1: none).  Not critical: enc_row[q] = -1.  Critical and enc_row[q] != p: event e = n_events[q]++ is
//      OPENED, enc_row[q] = p, and if e < capacity its record is written: ev_i32[q][e] = tick (open), tick (last), p, row_agent[p] (-1: a
//      scripted actor), path_off[q], path_off[row_agent[p]] (or -1), traj_idx[q], k_ttc; ev_f64[q][e] = c_now, state[q].v.  Critical and
//      enc_row[q] == p with a stored record (e = n_events[q] - 1 < capacity): word 1 = tick, word 7 = the smaller non-negative of itself
//      and k_ttc, ev_f64[0] = fmin(itself, c_now).  Last, always: tick[q]++.
// Every product and sum of step 2 is a statement of its own under "contract off" (host builds pass -ffp-contract=off): host and device
// agree bit for bit on every integer word; step 1 goes through sincos and hypot, which differ by a few ulp between the two.  tick, enc_row
// and n_events are device memory: a replayed hipGraph keeps counting.
#pragma once
#include <math.h>
#include "mpcx_record_core.h"

#if defined(__clang__)
#define MPCX_SAFETY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else       /* g++ honours no such pragma: a host build with it passes -ffp-contract=off */
#define MPCX_SAFETY_NO_CONTRACT
#endif

namespace mpcx {

constexpr int SAFETY_I32 = 8, SAFETY_F64 = 2;       // words of an event record
constexpr int SAFETY_SUM_I64 = 3, SAFETY_SUM_F64 = 2;       // columns of a cell of the conflict matrix

struct SafetyArgs {
    int P, n_pool, pred_steps;
    double radius, cc[4];                   // mpcx_interaction_params.radius / circle_centers
    const double *obs6;                     // n_pool x 6
    const double *pred;                     // n_pool x pred_steps x 4
    const double *state;                    // P x 4
    const int32_t *obs_off, *obs_cnt, *obs_skip;    // P each
    const int32_t *traj_idx, *path_off;     // P each
    const int32_t *done;                    // P or nullptr
    const int32_t *absent;                  // n_pool or nullptr
    mpcx_safety s;
};

// what the two searches leave of one agent
struct SafetyFound {
    int32_t r_now;                          // pool row of the nearest vehicle, -1: none
    double c_now;                           // its clearance, +inf: none
    int32_t r_ttc, k_ttc;                   // pool row and frame of the first predicted contact, -1: none
};

MPCX_REC_FN SafetyFound safety_none() { return SafetyFound{-1, (double)INFINITY, -1, -1}; }

// the agent is measured: the number of slots its window fills (0: not measured)
MPCX_REC_FN int safety_slots(const SafetyArgs &a, int q) {
    if (a.done && a.done[q] != 0) return 0;
    const int64_t own = a.obs_skip[q];
    if (own < 0 || own >= (int64_t)a.n_pool) return 0;
    if (a.absent && a.absent[own] != 0) return 0;
    const int64_t off = a.obs_off[q], cnt = a.obs_cnt[q];
    if (cnt <= 0) return 0;
    const int64_t others = cnt - (own >= off && own < off + cnt ? 1 : 0);
    return others < MPCX_MAX_OBS ? (int)others : MPCX_MAX_OBS;
}

// the pool row of slot j < safety_slots(): the window in row order with the agent's own row stepped over; -1: outside the pool or absent
MPCX_REC_FN int32_t safety_slot_row(const SafetyArgs &a, int q, int j) {
    const int64_t off = a.obs_off[q], own = a.obs_skip[q];
    int64_t r = off + j;
    if (own >= off && r >= own) r++;
    if (r < 0 || r >= (int64_t)a.n_pool) return -1;
    if (a.absent && a.absent[r] != 0) return -1;
    return (int32_t)r;
}

// step 1 for one other row: the smallest distance between a disc of the agent (ed, from rec_discs) and a disc of pool row r
MPCX_REC_FN double safety_now(const SafetyArgs &a, const double *ed, int32_t r) {
    const double *o = a.obs6 + 6 * (size_t)r;
    double od[4];
    rec_discs(a.cc, o[0], o[1], o[3], od);
    double best = INFINITY;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            best = fmin(best, hypot(ed[2 * i] - od[2 * j], ed[2 * i + 1] - od[2 * j + 1]));
    return best;
}

// step 2's measure, spelt as follow_d2
MPCX_REC_FN double safety_d2(double px, double py, double x, double y) {
    MPCX_SAFETY_NO_CONTRACT
    const double dx = px - x, dy = py - y;
    const double xx = dx * dx;
    const double yy = dy * dy;
    return xx + yy;
}

// (2 radius)^2
MPCX_REC_FN double safety_limit(const SafetyArgs &a) {
    MPCX_SAFETY_NO_CONTRACT
    const double two_r = 2.0 * a.radius;
    return two_r * two_r;
}

// step 2 for one other row: the lowest frame at which a disc of row o touches a disc of row r, -1: none
MPCX_REC_FN int32_t safety_contact(const SafetyArgs &a, int32_t o, int32_t r, double lim) {
    const double *po = a.pred + 4 * (size_t)a.pred_steps * (size_t)o, *pr = a.pred + 4 * (size_t)a.pred_steps * (size_t)r;
    for (int32_t k = 0; k < a.pred_steps; k++) {
        const double *e = po + 4 * (size_t)k, *f = pr + 4 * (size_t)k;
        double d = safety_d2(e[0], e[1], f[0], f[1]);
        const double d01 = safety_d2(e[0], e[1], f[2], f[3]);
        const double d10 = safety_d2(e[2], e[3], f[0], f[1]);
        const double d11 = safety_d2(e[2], e[3], f[2], f[3]);
        d = d01 < d ? d01 : d;
        d = d10 < d ? d10 : d;
        d = d11 < d ? d11 : d;
        if (d < lim) return k;
    }
    return -1;
}

// the owner of pool row p and its route: row_agent[p] if it names an agent, else -1 (a scripted actor)
MPCX_REC_FN int32_t safety_owner(const SafetyArgs &a, int32_t p) {
    if (p < 0 || p >= a.n_pool) return -1;
    const int32_t g = a.s.row_agent[p];
    return g >= 0 && g < a.P ? g : -1;
}

// steps 3 and 4 for agent q with what the searches found (safety_none(): not measured, or nobody there); every write of the stage
MPCX_REC_FN void safety_finish(const SafetyArgs &a, int q, const SafetyFound &f) {
    const mpcx_safety &s = a.s;
    s.partner[q] = f.r_now; s.clearance[q] = f.c_now; s.ttc_row[q] = f.r_ttc; s.ttc_frame[q] = f.k_ttc;
    const int32_t tick = s.tick[q];
    const bool close = f.r_now >= 0 && f.c_now < s.near;
    const bool soon = f.r_ttc >= 0 && f.k_ttc >= 0 && f.k_ttc < s.ttc_frames;
    if (!close && !soon) {
        s.enc_row[q] = -1;
    } else {
        const int32_t p = close ? f.r_now : f.r_ttc;
        if (s.enc_row[q] != p) {            // open
            const int32_t e = s.n_events[q];
            s.n_events[q] = e + 1;
            s.enc_row[q] = p;
            if (e >= 0 && e < s.capacity) {
                int32_t *w = s.ev_i32 + SAFETY_I32 * ((size_t)q * (size_t)s.capacity + (size_t)e);
                double *d = s.ev_f64 + SAFETY_F64 * ((size_t)q * (size_t)s.capacity + (size_t)e);
                const int32_t g = safety_owner(a, p);
                w[0] = tick; w[1] = tick; w[2] = p; w[3] = g;
                w[4] = a.path_off[q]; w[5] = g >= 0 ? a.path_off[g] : -1;
                w[6] = a.traj_idx[q]; w[7] = f.k_ttc;
                d[0] = f.c_now; d[1] = a.state[4 * (size_t)q + 2];
            }
        } else {                            // update
            const int32_t e = s.n_events[q] - 1;
            if (e >= 0 && e < s.capacity) {
                int32_t *w = s.ev_i32 + SAFETY_I32 * ((size_t)q * (size_t)s.capacity + (size_t)e);
                double *d = s.ev_f64 + SAFETY_F64 * ((size_t)q * (size_t)s.capacity + (size_t)e);
                w[1] = tick;
                if (f.k_ttc >= 0 && (w[7] < 0 || f.k_ttc < w[7])) w[7] = f.k_ttc;
                d[0] = fmin(d[0], f.c_now);
            }
        }
    }
    s.tick[q] = tick + 1;
}

// steps 1 and 2 of agent q on one lane (the host build; the kernel gives every slot a lane)
MPCX_REC_FN SafetyFound safety_search(const SafetyArgs &a, int q) {
    SafetyFound f = safety_none();
    const int n = safety_slots(a, q);
    if (n == 0) return f;
    const int32_t o = a.obs_skip[q];
    const double *e = a.obs6 + 6 * (size_t)o;
    double ed[4];
    rec_discs(a.cc, e[0], e[1], e[3], ed);
    const double lim = safety_limit(a);
    double best = INFINITY;
    for (int j = 0; j < n; j++) {
        const int32_t r = safety_slot_row(a, q, j);
        if (r < 0) continue;
        const double m = safety_now(a, ed, r);
        if (m < best) { best = m; f.r_now = r; }            // (slots rise: the first of equals stays)
        const int32_t k = safety_contact(a, o, r, lim);
        if (k >= 0 && (f.k_ttc < 0 || k < f.k_ttc)) { f.k_ttc = k; f.r_ttc = r; }
    }
    if (f.r_now >= 0) f.c_now = best - 2.0 * a.radius;
    return f;
}

// the stage for agent q on one lane
MPCX_REC_FN void safety_agent(const SafetyArgs &a, int q) { safety_finish(a, q, safety_search(a, q)); }

// ---- the conflict matrix.  The class of an event side is the route r with route_off[r] == its path_off word, the lowest r of equals; R: no
// route (an actor, or an unknown offset)
MPCX_REC_FN int safety_class(const int32_t *route_off, int R, int32_t off) {
    if (off >= 0)
        for (int r = 0; r < R; r++)
            if (route_off[r] == off) return r;
    return R;
}

// one stored event into a cell: acc = events, events with min clearance < 0, events with word 7 >= 0; lo = the minimum of min clearance (a
// NaN is skipped); k = the smallest word 7 >= 0 (INT32_MAX: none)
MPCX_REC_FN void safety_take(const int32_t *w, const double *d, int64_t *acc, double &lo, int32_t &k) {
    acc[0]++;
    if (d[0] < 0.0) acc[1]++;
    if (w[7] >= 0) { acc[2]++; if (w[7] < k) k = w[7]; }
    if (d[0] < lo) lo = d[0];
}

// the seconds of a smallest word 7 as safety_take left it
MPCX_REC_FN double safety_seconds(int32_t k, double dt) {
    MPCX_SAFETY_NO_CONTRACT
    if (k == INT32_MAX) return INFINITY;
    const double n = (double)k + 1.0;
    return n * dt;
}

}  // namespace mpcx
