// mpcx_follow_core.h -- CAR FOLLOWING: an agent keeps a standstill distance and a time gap to the car ahead of it on its own path.  Host +
// device source (the pattern of mpcx_signal_core.h and mpcx_advise_core.h).  follow_kernel (mpcx_follow.hip) runs it behind the signal /
// actuated / reserve stage of a closed-loop step (behind the conflict search where there are no signals), follow_clamp_kernel behind every
// window stage in speed mode; tests/follow_ref/follow_ref.cpp builds it for the host.
//
// The conflict search knows no leader: it pits a prediction of the car in front (its last controls held) against the ego's own
// full-throttle prediction and cuts the path where the two meet.  There is no standstill distance and no time gap in that, and in speed mode
// the position reference keeps pulling a follower towards a leader that brakes.  The rule is the signals' hold at a line that moves -- it
// lowers cut_len (the cut length, the stop index in speed mode) -- plus Gipps' safe speed as a cap on the speed reference.
//
// For agent q with done[q] == 0 (otherwise nothing but "no leader" is written: leader -1, gap -1.0, cap 0.0), reading traj_idx and cut_len
// as the stage before left them and obs6 as the head of this step packed it:
//   THE OTHERS: the rows of its pool window [obs_off[q], obs_off[q] + obs_cnt[q]) other than its own row obs_skip[q], in row order, the first
//      MPCX_MAX_OBS of them (slot j = 0 .. 15 <-> pool row follow_slot_row()); a row outside the pool or with absent[r] != 0 is left out.
//      Agents and scripted actors alike.  No window, ti = traj_idx[q] outside [0, path_len[q]): no leader.
//   1. PROJECTION.  k*(r) = the index k in [ti, min(ti + reach, path_len[q] - 1)] of q's FULL path that minimises dx dx + dy dy to (x_r, y_r);
//      on ties the lowest k.
//   2. CANDIDATE.  k*(r) > ti (beside or behind does not count); the minimum <= lateral^2; the row heads along the path there:
//      |wrap(yaw_path[k*] - yaw_r)| <= heading.  wrap: subtract / add 2 pi while above pi / below -pi, at most FOLLOW_WRAP_TURNS times -- every
//      subtraction is one correctly rounded operation, the same on host and device; a difference that is not finite or still outside
//      [-pi, pi] after that is refused.  No sin / cos: the device's differ from libm's and the decision must not.
//   3. LEADER.  The candidate with the smallest k*, on ties the lowest pool row (= the lowest slot).  leader[q] = its pool row, gap[q] =
//      (k* - ti) dl, v_l = max(obs6[r][2], 0).
//   4. STOP POINT, v = max(state[q][2], 0).  Cut mode: s = k* - ceil((standstill + time_gap v) / dl); speed mode: s = k* - ceil(standstill /
//      dl), the cap does the time gap there.  s is clamped to >= ti + 1 and cut_len[q] = min(cut_len[q], s): a shorter conflict cut or signal
//      hold is kept.
//   5. CAP (written in both modes, applied in speed mode): cap[q] = max(v_min, -b tau + sqrt(b^2 tau^2 + v_l^2 + 2 b max(gap - standstill, 0))),
//      b = brake, tau = time_gap: Gipps' safe speed.  0.0 = no leader.
//   6. CLAMP (speed mode, behind every window stage): every entry of row 2 of q's xref becomes fmin(entry, cap[q]) where cap[q] > 0; zeros
//      stay zero.  With advice on both clamps apply; a minimum of minima does not depend on their order.
// Every product and sum is a statement of its own under "contract off" (host builds pass -ffp-contract=off), sqrt, ceil and the divisions
// are correctly rounded: host and device agree bit for bit.  Precedence words are not consulted: a follower keeps its gap whoever has right
// of way.  Every write is to words of agent q and nothing the rule reads is written by it, so the outcome does not depend on the order of
// the lanes, and everything mutable is device memory: a replayed hipGraph behaves like a plain run.
#pragma once
#include <math.h>
#include "mpcx_record_core.h"

#if defined(__clang__)
#define MPCX_FOLLOW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else       /* g++ honours no such pragma: a host build with it passes -ffp-contract=off */
#define MPCX_FOLLOW_NO_CONTRACT
#endif

namespace mpcx {

constexpr int32_t FOLLOW_STEPS_MAX = 1 << 30;       // the clamp of the stop point's distance in points
constexpr int FOLLOW_WRAP_TURNS = 32;               // turns the heading test takes off a difference of yaws
constexpr double FOLLOW_TWO_PI = 6.283185307179586; // 2 * numpy.pi

struct FollowArgs {
    int P, W, n_pool;                       // agents; window points T + 1 (the clamp); pool rows
    int speed;                              // the stop mode is MPCX_STOP_SPEED
    double dl;
    const double *state;                    // P x 4
    const double *path_xyyaw;               // the path tables, 3 doubles a point
    const int32_t *path_off, *path_len;     // P each
    const int32_t *traj_idx;                // P, as the conflict search left it
    int32_t *cut_len;                       // P, in-out
    const int32_t *done;                    // P or nullptr
    const double *obs6;                     // n_pool x 6
    const int32_t *obs_off, *obs_cnt, *obs_skip;    // P each (obs_skip or nullptr: no row of its own)
    const int32_t *absent;                  // n_pool or nullptr
    double *xref;                           // P x 4 x W (the clamp)
    mpcx_following fl;
};

// what the search leaves of one agent
struct FollowLeader {
    int32_t row, k;                         // pool row (-1: none) and k* of the leader
    double v;                               // obs6[row][2]
};

// the agent takes part: the number of slots its window fills (0: no leader, whatever else holds)
MPCX_REC_FN int follow_slots(const FollowArgs &a, int q) {
    if (a.done && a.done[q] != 0) return 0;
    const int32_t ti = a.traj_idx[q];
    if (ti < 0 || ti >= a.path_len[q]) return 0;
    const int32_t off = a.obs_off[q], cnt = a.obs_cnt[q], own = a.obs_skip ? a.obs_skip[q] : -1;
    if (cnt <= 0) return 0;
    const int64_t others = (int64_t)cnt - ((int64_t)own >= (int64_t)off && (int64_t)own < (int64_t)off + (int64_t)cnt ? 1 : 0);
    return others < MPCX_MAX_OBS ? (int)others : MPCX_MAX_OBS;
}

// the pool row of slot j < follow_slots(): the window in row order with the agent's own row stepped over; -1: outside the pool or absent
MPCX_REC_FN int32_t follow_slot_row(const FollowArgs &a, int q, int j) {
    const int64_t off = a.obs_off[q], own = a.obs_skip ? a.obs_skip[q] : -1;
    int64_t r = off + j;
    if (own >= off && r >= own) r++;
    if (r < 0 || r >= (int64_t)a.n_pool) return -1;
    if (a.absent && a.absent[r] != 0) return -1;
    return (int32_t)r;
}

// the last path index the projection scans
MPCX_REC_FN int32_t follow_last(const FollowArgs &a, int q) {
    const int64_t ti = a.traj_idx[q], end = ti + (int64_t)a.fl.reach, lim = (int64_t)a.path_len[q] - 1;
    return (int32_t)(end < lim ? end : lim);
}

// step 1's measure
MPCX_REC_FN double follow_d2(double px, double py, double x, double y) {
    MPCX_FOLLOW_NO_CONTRACT
    const double dx = px - x, dy = py - y;
    const double xx = dx * dx;
    const double yy = dy * dy;
    return xx + yy;
}

// step 2 for a row whose projection is (d2, k) onto a point of heading yaw_path
MPCX_REC_FN bool follow_candidate(const FollowArgs &a, int32_t ti, double d2, int32_t k, double yaw_path, double yaw_row) {
    MPCX_FOLLOW_NO_CONTRACT
    if (k <= ti) return false;
    const double lat2 = a.fl.lateral * a.fl.lateral;
    if (!(d2 <= lat2)) return false;
    double w = yaw_path - yaw_row;
    if (!(fabs(w) <= (double)(FOLLOW_WRAP_TURNS + 1) * FOLLOW_TWO_PI)) return false;       // (also a NaN)
    for (int i = 0; i < FOLLOW_WRAP_TURNS + 1 && w > REC_PI; i++) w = w - FOLLOW_TWO_PI;
    for (int i = 0; i < FOLLOW_WRAP_TURNS + 1 && w < -REC_PI; i++) w = w + FOLLOW_TWO_PI;
    return fabs(w) <= a.fl.heading;
}

// steps 3's outputs, 4 and 5 for agent q with the leader the search found (row < 0: none); every write of the search stage
MPCX_REC_FN void follow_finish(const FollowArgs &a, int q, const FollowLeader &ld) {
    MPCX_FOLLOW_NO_CONTRACT
    const mpcx_following &f = a.fl;
    if (ld.row < 0) {
        f.leader[q] = -1; f.gap[q] = -1.0; f.cap[q] = 0.0;
        return;
    }
    const int32_t ti = a.traj_idx[q];
    const double gap = (double)(ld.k - ti) * a.dl;
    const double vl = ld.v > 0.0 ? ld.v : 0.0;
    const double ve = a.state[4 * (size_t)q + 2];
    const double v = ve > 0.0 ? ve : 0.0;
    // 4. the stop point
    double need = f.standstill;
    if (!a.speed) {
        const double tv = f.time_gap * v;
        need = f.standstill + tv;
    }
    const double nd = ceil(need / a.dl);
    const int32_t n = nd < (double)FOLLOW_STEPS_MAX ? (int32_t)nd : FOLLOW_STEPS_MAX;         // (NaN: the clamp)
    int64_t s = (int64_t)ld.k - (int64_t)n;
    if (s < (int64_t)ti + 1) s = (int64_t)ti + 1;
    if (s < (int64_t)a.cut_len[q]) a.cut_len[q] = (int32_t)s;
    // 5. Gipps' safe speed
    const double over = gap - f.standstill;
    const double room = over > 0.0 ? over : 0.0;
    const double bt = f.brake * f.time_gap;
    const double bt2 = bt * bt;
    const double vl2 = vl * vl;
    const double b2 = 2.0 * f.brake;
    const double br = b2 * room;
    const double sum1 = bt2 + vl2;
    const double sum = sum1 + br;
    const double vs = sqrt(sum) - bt;
    f.leader[q] = ld.row; f.gap[q] = gap; f.cap[q] = vs > f.v_min ? vs : f.v_min;
}

// the search of agent q on one lane (the host build; the kernel spreads the scan over a lane group): steps 1 - 3
MPCX_REC_FN FollowLeader follow_search(const FollowArgs &a, int q) {
    FollowLeader best{-1, 0, 0.0};
    const int n = follow_slots(a, q);
    if (n == 0) return best;
    const int32_t ti = a.traj_idx[q], last = follow_last(a, q);
    const double *path = a.path_xyyaw + 3 * (size_t)a.path_off[q];
    for (int j = 0; j < n; j++) {
        const int32_t r = follow_slot_row(a, q, j);
        if (r < 0) continue;
        const double *o = a.obs6 + 6 * (size_t)r;
        double d2 = INFINITY;
        int32_t ks = ti;
        for (int32_t k = ti; k <= last; k++) {
            const double d = follow_d2(path[3 * (size_t)k], path[3 * (size_t)k + 1], o[0], o[1]);
            if (d < d2) { d2 = d; ks = k; }
        }
        if (!follow_candidate(a, ti, d2, ks, path[3 * (size_t)ks + 2], o[3])) continue;
        if (best.row < 0 || ks < best.k) best = FollowLeader{r, ks, o[2]};       // (slots rise with the pool row: the first of equals stays)
    }
    return best;
}

// the search stage for agent q on one lane; returns leader[q]
MPCX_REC_FN int32_t follow_agent(const FollowArgs &a, int q) {
    const FollowLeader ld = follow_search(a, q);
    follow_finish(a, q, ld);
    return ld.row;
}

// step 6 for window point t of agent q under the cap v (> 0)
MPCX_REC_FN void follow_clamp(const FollowArgs &a, int q, int t, double v) {
    double *e = a.xref + ((size_t)4 * (size_t)q + 2) * (size_t)a.W + (size_t)t;
    *e = fmin(*e, v);
}

// the clamp stage for agent q on one lane (the host build)
MPCX_REC_FN void follow_clamp_agent(const FollowArgs &a, int q) {
    if (a.done && a.done[q] != 0) return;
    const double v = a.fl.cap[q];
    if (v > 0.0)
        for (int t = 0; t < a.W; t++) follow_clamp(a, q, t, v);
}

}  // namespace mpcx
