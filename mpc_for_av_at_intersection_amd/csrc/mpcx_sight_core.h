// mpcx_sight_core.h -- LINE OF SIGHT: buildings hide cars from each other.  Host + device source (the pattern of mpcx_follow_core.h and
// mpcx_safety_core.h).  sight_kernel (mpcx_sight.hip) runs it once per closed-loop step behind the pack of the pool and the intent stage and
// in front of the conflict search, whose SIGHT instantiations AND its word onto their ballot of present rows;
// tests/sight_ref/sight_ref.cpp builds it for the host.
//
// For agent q with own row o = obs_skip[q], window [obs_off[q], obs_off[q] + obs_cnt[q]) and eye E = (state[q].x, state[q].y), and for
// window offset j < min(obs_cnt[q], 64) with row r = obs_off[q] + j:
//   NOT A CANDIDATE   r outside the pool, r == o, or absent[r] != 0 (absent given): bit j = 0, the row is not counted.
//   OUT OF RANGE      dx dx + dy dy > range range with (dx, dy) = T - E, T = the (x, y) of obs6[r]: hidden.  No trig, no car extent: the
//                     reference point stands for the car.
//   HEARD             in range and heard[r] != 0 (heard given): seen, the occluders are not consulted -- a connected vehicle announces
//                     its pose.
//   OTHERWISE         seen iff no occluder of the agent's set blocks the segment E -> T.
// OCCLUDERS are convex polygons as half-plane rows (a, b, c), inside <=> a x + b y + c <= 0, stored CSR: occluder i has the rows
// hp[3 hp_off[i] .. 3 hp_off[i + 1]) and a bounding box box[4 i ..] = (x0, y0, x1, y1) computed by the host.  The agent's SET is
// set_of[q]: the occluders set_off[s] .. set_off[s + 1); a value outside [0, n_sets) is the empty set (the host checks set_of; the rule
// never reads outside the tables for a bad word).
//   1. BOX CULL.  The occluder is skipped if the segment's own box does not overlap its box: max(Ex, Tx) < x0, min(Ex, Tx) > x1, and the
//      same in y -- four comparisons, part of the rule.
//   2. CYRUS-BECK.  t_in = 0, t_out = 1; per row den = a dx + b dy, num = -((a Ex + b Ey) + c).  den == 0 and num < 0: the segment is outside
//      this polygon, which is finished.  den > 0: t_out = min(t_out, num / den).  den < 0: t_in = max(t_in, num / den).  The occluder blocks
//      iff it was not left early and t_in < t_out.  Strict: a grazing segment is not blocked.  An eye or a target inside an occluder is
//      blocked; T == E is blocked iff E is inside.  An occluder without rows is the whole plane.
// OUTPUTS, every one a word of agent q: sight[q] bit j = the row at window offset j is seen; n_seen[q] = its population count; n_hidden[q] =
// the candidates that are not seen.  A retired agent (done[q] != 0) writes 0, 0, 0.
// Every product and sum is a statement of its own under "contract off" (host builds pass -ffp-contract=off) and the division is correctly
// rounded: host, device and the numpy restatement agree bit for bit.  A NaN fails every comparison alike in all three.
#pragma once
#include <math.h>
#include "mpcx_record_core.h"

#if defined(__clang__)
#define MPCX_SIGHT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else       /* g++ honours no such pragma: a host build with it passes -ffp-contract=off */
#define MPCX_SIGHT_NO_CONTRACT
#endif

namespace mpcx {

constexpr int SIGHT_WINDOW = 64;            // window offsets a word holds

struct SightArgs {
    int P, n_pool;
    const double *state;                    // P x 4
    const double *obs6;                     // n_pool x 6
    const int32_t *obs_off, *obs_cnt, *obs_skip;    // P each
    const int32_t *done;                    // P or nullptr
    const int32_t *absent;                  // n_pool or nullptr
    mpcx_sight s;
};

// the window offsets of agent q that the word covers
MPCX_REC_FN int sight_window(const SightArgs &a, int q) {
    const int32_t cnt = a.obs_cnt[q];
    return cnt <= 0 ? 0 : cnt < SIGHT_WINDOW ? (int)cnt : SIGHT_WINDOW;
}

// the pool row at window offset j of agent q if it is a candidate, else -1
MPCX_REC_FN int32_t sight_candidate(const SightArgs &a, int q, int j) {
    const int64_t r = (int64_t)a.obs_off[q] + (int64_t)j;
    if (r < 0 || r >= (int64_t)a.n_pool || r == (int64_t)a.obs_skip[q]) return -1;
    if (a.absent && a.absent[r] != 0) return -1;
    return (int32_t)r;
}

// the occluders [first, last) of agent q's set; a word outside [0, n_sets) is the empty set
MPCX_REC_FN void sight_set(const SightArgs &a, int q, int32_t &first, int32_t &last) {
    const int32_t s = a.s.set_of[q];
    first = last = 0;
    if (s < 0 || s >= a.s.n_sets) return;
    first = a.s.set_off[s]; last = a.s.set_off[s + 1];
}

// step 1: the box of the segment E -> T misses the occluder's box (x0, y0, x1, y1)
MPCX_REC_FN bool sight_culled(const double *box, double ex, double ey, double tx, double ty) {
    const double sx0 = ex < tx ? ex : tx, sx1 = ex < tx ? tx : ex;
    const double sy0 = ey < ty ? ey : ty, sy1 = ey < ty ? ty : ey;
    return sx1 < box[0] || sx0 > box[2] || sy1 < box[1] || sy0 > box[3];
}

// step 2: the polygon of n rows (a, b, c) blocks the segment from E along d = T - E
MPCX_REC_FN bool sight_blocks(const double *hp, int32_t n, double ex, double ey, double dx, double dy) {
    MPCX_SIGHT_NO_CONTRACT
    double t_in = 0.0, t_out = 1.0;
    for (int32_t k = 0; k < n; k++) {
        const double ha = hp[3 * (size_t)k], hb = hp[3 * (size_t)k + 1], hc = hp[3 * (size_t)k + 2];
        const double adx = ha * dx;
        const double bdy = hb * dy;
        const double den = adx + bdy;
        const double aex = ha * ex;
        const double bey = hb * ey;
        const double lin = aex + bey;
        const double val = lin + hc;
        const double num = -val;
        if (den == 0.0) {
            if (num < 0.0) return false;
        } else if (den > 0.0) {
            const double t = num / den;
            t_out = t < t_out ? t : t_out;
        } else if (den < 0.0) {
            const double t = num / den;
            t_in = t > t_in ? t : t_in;
        }
    }
    return t_in < t_out;
}

// candidate row r is seen by agent q whose set is the occluders [first, last)
MPCX_REC_FN bool sight_sees(const SightArgs &a, int q, int32_t r, int32_t first, int32_t last) {
    MPCX_SIGHT_NO_CONTRACT
    const double ex = a.state[4 * (size_t)q], ey = a.state[4 * (size_t)q + 1];
    const double tx = a.obs6[6 * (size_t)r], ty = a.obs6[6 * (size_t)r + 1];
    const double dx = tx - ex, dy = ty - ey;
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double d2 = xx + yy;
    const double r2 = a.s.range * a.s.range;
    if (d2 > r2) return false;
    if (a.s.heard && a.s.heard[r] != 0) return true;
    for (int32_t i = first; i < last; i++) {
        if (sight_culled(a.s.box + 4 * (size_t)i, ex, ey, tx, ty)) continue;
        const int32_t h0 = a.s.hp_off[i], h1 = a.s.hp_off[i + 1];
        if (sight_blocks(a.s.hp + 3 * (size_t)h0, h1 - h0, ex, ey, dx, dy)) return false;
    }
    return true;
}

// every write of the stage for agent q
MPCX_REC_FN void sight_write(const SightArgs &a, int q, unsigned long long seen, unsigned long long candidates) {
    a.s.sight[q] = (uint64_t)seen;
    a.s.n_seen[q] = (int32_t)__builtin_popcountll(seen);
    a.s.n_hidden[q] = (int32_t)__builtin_popcountll(candidates & ~seen);
}

// the stage for agent q on one lane (the host build; the kernel gives every window offset a lane)
MPCX_REC_FN void sight_agent(const SightArgs &a, int q) {
    unsigned long long seen = 0ull, cand = 0ull;
    if (!(a.done && a.done[q] != 0)) {
        int32_t first, last;
        sight_set(a, q, first, last);
        const int n = sight_window(a, q);
        for (int j = 0; j < n; j++) {
            const int32_t r = sight_candidate(a, q, j);
            if (r < 0) continue;
            cand |= 1ull << j;
            if (sight_sees(a, q, r, first, last)) seen |= 1ull << j;
        }
    }
    sight_write(a, q, seen, cand);
}

}  // namespace mpcx
