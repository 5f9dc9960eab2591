// mpcx_stopsign_core.h -- STOP SIGNS: an agent of a signed movement comes to a standstill at its stop line, and the agents that have
// stopped leave in the order in which they stopped; in the two-way case a stopped agent also waits for a gap in the unsigned road.  Host +
// device source (the pattern of mpcx_priority_core.h, whose eta expression and -- through it -- keep clear's classification it calls).
// stopsign_kernel (mpcx_stopsign.hip) runs it with a lane group per junction in the hold's place -- behind the conflict search and the
// safety stage, in front of the following stage; tests/stopsign_ref/stopsign_ref.cpp builds it for the host.
//
// There are no signals in the run: the stop line, the movement and the exit point of a path point are the stage's own tables.  A junction is
// n_per consecutive agents (n_per <= 64): junction j owns agents [j n_per, (j + 1) n_per).  Tables: path_stop[n_points], path_move[n_points],
// path_exit[n_points] as the priority road's; conflict[n_moves] bit h of word g = movements g and h cross (symmetric, no self-bit);
// lane[n_moves] bit h of word g = they queue in the same approach lane (bit g of word g is set); sign[n_moves] 0 = uncontrolled, 1 = stop
// sign; gap[n_moves] the critical gap in seconds of a signed movement against unsigned traffic (finite, >= 0).  Scalars: v_stop (> 0, a car
// at or below this speed stands), zone (>= 1, path points before the line within which a standstill counts as the stop), detect (>= zone),
// brake (> 0), v_floor (> 0), patience (>= 0, steps).  State, in-out: stopped_at[P] (the junction clock at which the agent completed its
// stop, -1 = not yet; -1-initialised), go[P] (0 / 1), stopping[P] (0 / 1: the hold word, and last step's stickiness), clock[n_junctions],
// ran[n_junctions] (a running count), all zero-initialised.  Out: lag[P], blocker[P], occupied[n_junctions], n_waiting[n_junctions].
//
// Per junction and step, everything is read before anything is written:
//   1. t = clock[j], a negative word counts as 0; clock[j] = t + 1 (the reservation's wrapping into the negative words).
//   2. every agent q is OUT, INSIDE or APPROACH with (m, s, ti) as keepclear_classify decides on the stage's tables; d = s - ti in 64 bits.
//      OUT: go = 0, stopped_at = -1, stopping = 0.
//      INSIDE: it occupies m.  If sign[m] != 0 and go == 0 it RAN the sign: ran[j] += 1 (once: then go = 1).  stopped_at is left alone,
//         stopping = 0.
//      APPROACH, sign[m] == 0: never held; go = 0, stopped_at = -1, stopping = 0.  eta = (double)d * dl / fmax(v, v_floor) (priority_eta)
//         is what signed agents see of it in step 4.
//      APPROACH, signed, go != 0: it occupies m -- a release is never revoked; stopped_at is left alone, stopping = 0.
//      APPROACH, signed, go == 0, d > detect: stopped_at = -1, stopping = 0.
//      APPROACH, signed, go == 0, d <= detect: SUBJECT.  If stopped_at < 0, d <= zone and v <= v_stop: stopped_at = t.  A subject agent
//         with stopped_at >= 0 REQUESTS.
//   3. occ = OR of 1 << m over the occupying agents.
//   4. a requester q: lag[q] = the lexicographic minimum of (eta_r, r) over the unsigned APPROACH agents r of the junction with bit m_r of
//      conflict[m_q] set, blocker[q] = the agent that attains it; none: +inf and -1.  Everybody else: lag = +inf, blocker = -1.
//   5. the requesters in ascending order of (stopped_at, index within the junction), from ahead = blocked = 0: a requester of movement m is
//      RELEASED (go = 1, occ |= 1 << m) if (conflict[m] & (occ | blocked)) == 0, (lane[m] & ahead) == 0 and lag >= gap[m]; otherwise it is
//      denied, ahead |= 1 << m, and if it is aged, (int64)t - stopped_at >= patience, also blocked |= 1 << m.  So a car that stopped later
//      and conflicts with no earlier one may go, and a conflicting one may not jump an aged one.
//   6. a subject agent with go == 0 after step 5 is HELD if stopping[q] != 0 from the step before, or if it can still stop, (double)d * dl
//      >= v * v / (2.0 * brake) -- signal_hold's expression.  Held: stopping = 1, cut_len = min(cut_len, s).  Otherwise stopping = 0: the
//      car is left to the conflict search, and ran will count it.
//   7. occupied[j] = occ, n_waiting[j] = the number of agents with stopping != 0.
// The order of step 5 is one 64-bit key per requester, stopped_at << 32 | index << 16 | (lag >= gap[m]) << 8 | m, and a loop of minima: the
// host walks an array, the kernel a lane group, as the reservation's grant loop does.  The only floating point is the eta division, the
// two speed comparisons (v <= v_stop, lag >= gap) and the can-stop comparison; nothing can fuse, host builds use -ffp-contract=off all the
// same.  A NaN speed counts as v_floor in eta (fmax), never stamps and cannot stop.
//
// What the order implies: cut_len is only lowered, so a conflict cut in front of the line is kept; the stage writes no word of another
// stage.  A vehicle that arrives has been OUT since its exit point and a slot reset by the respawn stage is OUT while it waits at the gate
// (done[q] != 0), so step 2 has reset go, stopped_at and stopping (and step 4 lag and blocker) before the next vehicle drives: the words
// heal themselves.  The outcome depends neither on the order of the junctions nor on that of the lanes, and a replayed hipGraph counts
// like a plain run.
#pragma once
#include "mpcx_priority_core.h"
#include "mpcx_reserve_core.h"
#include <cmath>
#include <cstdint>

#define MPCX_STOPSIGN_NO_KEY 0xffffffffffffffffull      /* the key of an agent that does not request */

namespace mpcx {

struct StopSignArgs {
    SignalArgs s;           // the hold's words; of s.sg only path_stop is set (the stage's own table): what keepclear_classify reads
    mpcx_stopsign ss;
};

// an agent as step 2 leaves it
struct StopSignAgent {
    int32_t m, s;           // the movement (INSIDE, APPROACH); the line (APPROACH)
    int32_t um;             // the movement of an unsigned APPROACH agent, -1 for everybody else: what the others see of it, with eta
    int32_t go, stopped_at; // the two words as step 2 leaves them
    int32_t ran;            // 1 = the agent ran the sign in this step
    int32_t subject;        // 1 = signed APPROACH inside the detector without a release
    uint32_t occ;           // its bit in occ
    uint32_t cf;            // conflict[m] (a subject agent)
    int64_t d;              // s - ti (APPROACH; 64 bits: a defective negative traj_idx does not overflow it)
    double eta;             // seconds to the line (an unsigned APPROACH agent)
};

// step 2 for agent q at junction time t
MPCX_REC_FN StopSignAgent stopsign_classify(const StopSignArgs &a, int q, int32_t t) {
    const mpcx_stopsign &k = a.ss;
    const mpcx_keepclear view{k.path_move, k.path_exit, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, k.n_moves, k.n_points, 0};
    const KeepClearAgent c = keepclear_classify(a.s, view, q);
    StopSignAgent p{c.m, c.s, -1, 0, -1, 0, 0, 0u, 0u, 0, 0.0};
    if (c.kind == MPCX_KEEPCLEAR_OUT) return p;
    const int32_t go = k.go[q], sign = k.sign[c.m];
    const uint32_t bit = 1u << c.m;
    if (c.kind == MPCX_KEEPCLEAR_INSIDE) {
        p.ran = sign != 0 && go == 0 ? 1 : 0;
        p.go = 1;
        p.stopped_at = k.stopped_at[q];
        p.occ = bit;
        return p;
    }
    p.d = (int64_t)c.s - (int64_t)c.ti;
    const double v = a.s.state[4 * (size_t)q + 2];
    if (sign == 0) {
        p.um = c.m;
        p.eta = priority_eta(p.d, a.s.dl, v, k.v_floor);
        return p;
    }
    if (go != 0) {
        p.go = go;
        p.stopped_at = k.stopped_at[q];
        p.occ = bit;
        return p;
    }
    if (p.d > (int64_t)k.detect) return p;
    p.subject = 1;
    p.cf = (uint32_t)k.conflict[c.m];
    p.stopped_at = k.stopped_at[q];
    if (p.stopped_at < 0) p.stopped_at = p.d <= (int64_t)k.zone && v <= k.v_stop ? t : -1;
    return p;
}

// a subject agent with a stamp requests
MPCX_REC_FN bool stopsign_requests(const StopSignAgent &p) { return p.subject != 0 && p.stopped_at >= 0; }

// step 4, one other agent r (um_r, eta_r) seen by agent q: keeps the lexicographic minimum of (eta, index) over the unsigned APPROACH
// agents that cross q's movement in (lag, blocker), which start as (+inf, -1)
MPCX_REC_FN void stopsign_meet(const StopSignAgent &me, int32_t um_r, double eta_r, int32_t r, double &lag, int32_t &blocker) {
    if (um_r >= 0 && ((me.cf >> um_r) & 1u) != 0 && (eta_r < lag || (eta_r == lag && (blocker < 0 || r < blocker)))) {
        lag = eta_r;
        blocker = r;
    }
}

// step 5: the key of the agent at place idx of its junction with the lag it met, MPCX_STOPSIGN_NO_KEY unless it requests
MPCX_REC_FN uint64_t stopsign_key(const mpcx_stopsign &k, const StopSignAgent &p, int idx, double lag) {
    if (!stopsign_requests(p)) return MPCX_STOPSIGN_NO_KEY;
    const uint32_t gap_ok = lag >= k.gap[p.m] ? 1u : 0u;
    return (uint64_t)(uint32_t)p.stopped_at << 32 | (uint64_t)(uint32_t)idx << 16 | (uint64_t)gap_ok << 8 | (uint64_t)(uint32_t)p.m;
}

// step 5: the masks of the release loop, and the requester with the smallest key left decided on them; released = the last decision
struct StopSignMasks {
    uint32_t occ, ahead, blocked;
    bool released;
};
MPCX_REC_FN StopSignMasks stopsign_decide(const mpcx_stopsign &k, uint64_t key, int32_t t, StopSignMasks m) {
    const int32_t g = (int32_t)(key & 0xffu), stamp = (int32_t)(key >> 32);
    const uint32_t bit = 1u << g;
    m.released = ((uint32_t)k.conflict[g] & (m.occ | m.blocked)) == 0 && ((uint32_t)k.lane[g] & m.ahead) == 0 && ((key >> 8) & 1u) != 0;
    if (m.released) {
        m.occ |= bit;
    } else {
        m.ahead |= bit;
        if ((int64_t)t - (int64_t)stamp >= (int64_t)k.patience) m.blocked |= bit;
    }
    return m;
}

// steps 4 and 6 for agent q and the writes of its own words: p as the release loop left it (p.go = 1 for a released requester), the lag
// it met; returns stopping[q]
MPCX_REC_FN int32_t stopsign_agent(const StopSignArgs &a, int q, const StopSignAgent &p, double lag, int32_t blocker) {
    const mpcx_stopsign &k = a.ss;
    int32_t stopping = 0;
    if (p.subject != 0 && p.go == 0) {
        const double v = a.s.state[4 * (size_t)q + 2];
        if (k.stopping[q] != 0 || (double)p.d * a.s.dl >= v * v / (2.0 * k.brake)) stopping = 1;
        if (stopping != 0 && p.s < a.s.cut_len[q]) a.s.cut_len[q] = p.s;
    }
    const bool asked = stopsign_requests(p);
    k.lag[q] = asked ? lag : (double)INFINITY;
    k.blocker[q] = asked ? blocker : -1;
    k.go[q] = p.go;
    k.stopped_at[q] = p.stopped_at;
    k.stopping[q] = stopping;
    return stopping;
}

// the whole rule for junction j as loops (the host's order; the kernel spreads the agents over a lane group); returns the agents waiting
MPCX_REC_FN int stopsign_junction(const StopSignArgs &a, int j) {
    const mpcx_stopsign &k = a.ss;
    const int n = k.n_per < 64 ? k.n_per : 64;
    const int q0 = j * k.n_per;
    const int32_t t = reserve_clock(k.clock[j]);
    StopSignAgent ag[64];
    double lag[64];
    int32_t blocker[64];
    uint64_t key[64];
    StopSignMasks mk{0u, 0u, 0u, false};
    int32_t ran = 0;
    for (int m = 0; m < n; m++) {
        ag[m] = stopsign_classify(a, q0 + m, t);
        mk.occ |= ag[m].occ;
        ran += ag[m].ran;
    }
    for (int m = 0; m < n; m++) {
        lag[m] = INFINITY;
        blocker[m] = -1;
        for (int r = 0; r < n; r++)
            if (r != m) stopsign_meet(ag[m], ag[r].um, ag[r].eta, q0 + r, lag[m], blocker[m]);
        key[m] = stopsign_key(k, ag[m], m, lag[m]);
    }
    for (;;) {
        int w = -1;
        for (int m = 0; m < n; m++)
            if (key[m] != MPCX_STOPSIGN_NO_KEY && (w < 0 || key[m] < key[w])) w = m;
        if (w < 0) break;
        mk = stopsign_decide(k, key[w], t, mk);
        if (mk.released) ag[w].go = 1;
        key[w] = MPCX_STOPSIGN_NO_KEY;
    }
    int got = 0;
    for (int m = 0; m < n; m++) got += stopsign_agent(a, q0 + m, ag[m], lag[m], blocker[m]);
    k.clock[j] = reserve_tick(t);
    k.ran[j] = (int32_t)((uint32_t)k.ran[j] + (uint32_t)ran);
    k.occupied[j] = (int32_t)mk.occ;
    k.n_waiting[j] = got;
    return got;
}

}  // namespace mpcx
