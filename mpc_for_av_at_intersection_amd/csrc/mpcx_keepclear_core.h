// mpcx_keepclear_core.h -- KEEP CLEAR: an agent whose light lets it go is held at its stop line while a movement that conflicts with its
// own is inside the crossing.  Host + device source (the pattern of mpcx_reserve_core.h, whose classification it shares word for word).
// keepclear_kernel (mpcx_keepclear.hip) runs it with a lane group per junction directly behind signal_kernel / actuated_signal_kernel and
// in front of the following stage; tests/keepclear_ref/keepclear_ref.cpp builds it for the host.
//
// The signal groups stay what they are (arms): the stop line, held and brake are read from the run's mpcx_signals.  The MOVEMENT of an
// agent comes from the stage's own table.  A junction is n_per consecutive agents (n_per <= 64): junction j owns agents [j n_per,
// (j + 1) n_per).  Tables: path_move[n_points] the movement of the route on that path point (at most MPCX_SIGNAL_GROUPS_MAX movements);
// path_exit[n_points] the route-local index e at which a vehicle on this point has left the crossing (-1: no crossing ahead or under the
// point); conflict[n_moves] bit h of word g = movements g and h may not be in the crossing together (symmetric, no self-bit).  State:
// waited[P] in-out, zero-initialised; out: boxed[P] (0 / 1), occupied[n_junctions], n_boxed[n_junctions].
//
// Per junction and step, in this order:
//   1. every agent q, with ti = traj_idx[q] as the conflict search left it, i = path_off[q] + ti, s = path_stop[i], m = path_move[i], e =
//      path_exit[i]: OUT: done[q] != 0 (retired, or waiting for admission); i outside [0, n_points); e < 0, e > path_len[q] or ti >= e; m
//      outside [0, n_moves); or ti < s with s >= path_len[q].  INSIDE: not OUT and (s < 0 or ti >= s).  APPROACH: ti < s.
//   2. occ = OR of 1 << m over the INSIDE agents.
//   3. an APPROACH agent is a CANDIDATE if held[q] == 0 as this step's hold left it, s - ti <= detect and (conflict[m] & occ) != 0.  A
//      candidate is BOXED if waited[q] != 0 (a car that stood at its line in the step before does not start into an occupied box: the amber
//      rule's stickiness) or if it can stop, (double)(s - ti) * dl >= v * v / (2.0 * brake), v = state[q][2] -- signal_hold's expression.
//      Otherwise it is free: a car that arrives at speed on green and cannot stop any more is left to the conflict search, as on amber.
//      Boxed: boxed[q] = 1, cut_len[q] = min(cut_len[q], s).  Everybody else: boxed[q] = 0, cut_len untouched.
//   4. waited[q] = 1 for an APPROACH agent with held[q] != 0 or boxed[q] != 0, 0 for everybody else.
//   5. occupied[j] = occ, n_boxed[j] = the number boxed.
// The comparison of step 3 is the only floating point; it has no multiply-add to fuse, host builds use -ffp-contract=off all the same.
//
// What the order implies: held is read only and stays the signal stage's word; cut_len is only lowered, so a conflict cut or a hold in front
// of the line is kept; the stage writes no word of another stage.  A vehicle that arrives has been OUT since its exit point, and a slot reset
// by the respawn stage is OUT while it waits at the gate (done[q] != 0), so step 4 has cleared its waited word before the next vehicle
// drives: the word heals itself and the respawn stages need not know it.  A junction's words are read before any of them is written and its agents' words are the agents' own: the outcome depends
// neither on the order of the junctions nor on that of the lanes, and a replayed hipGraph counts like a plain run.
#pragma once
#include "mpcx_signal_core.h"

#define MPCX_KEEPCLEAR_OUT 0
#define MPCX_KEEPCLEAR_INSIDE 1
#define MPCX_KEEPCLEAR_APPROACH 2

namespace mpcx {

struct KeepClearArgs {
    SignalArgs s;           // the hold's words: s.sg supplies path_stop, held, brake
    mpcx_keepclear kc;
};

struct KeepClearAgent {
    int32_t kind, m, s, ti; // MPCX_KEEPCLEAR_*; the movement (INSIDE, APPROACH); the line and the index (APPROACH)
};

// step 1: where agent q stands (reserve_classify with path_move in the place of path_group)
MPCX_REC_FN KeepClearAgent keepclear_classify(const SignalArgs &a, const mpcx_keepclear &k, int q) {
    KeepClearAgent c{MPCX_KEEPCLEAR_OUT, 0, 0, 0};
    if (a.done && a.done[q] != 0) return c;
    const int32_t ti = a.traj_idx[q];
    const int64_t i = (int64_t)a.path_off[q] + (int64_t)ti;
    if (i < 0 || i >= (int64_t)k.n_points) return c;
    const int32_t s = a.sg.path_stop[i], m = k.path_move[i], e = k.path_exit[i];
    if (e < 0 || e > a.path_len[q] || ti >= e || m < 0 || m >= k.n_moves) return c;
    c.m = m;
    if (s < 0 || ti >= s) { c.kind = MPCX_KEEPCLEAR_INSIDE; return c; }
    if (s >= a.path_len[q]) return c;
    c.kind = MPCX_KEEPCLEAR_APPROACH;
    c.s = s;
    c.ti = ti;
    return c;
}

// step 2: the agent's bit in occ
MPCX_REC_FN uint32_t keepclear_occupies(const KeepClearAgent &c) { return c.kind == MPCX_KEEPCLEAR_INSIDE ? 1u << c.m : 0u; }

// steps 3 and 4 for agent q on the junction's occ: writes boxed[q] and waited[q], lowers cut_len[q]; returns boxed[q]
MPCX_REC_FN int32_t keepclear_agent(const SignalArgs &a, const mpcx_keepclear &k, int q, const KeepClearAgent &c, uint32_t occ) {
    int32_t boxed = 0, waited = 0;
    if (c.kind == MPCX_KEEPCLEAR_APPROACH) {
        const int32_t held = a.sg.held[q];
        const int64_t d = (int64_t)c.s - (int64_t)c.ti;     // (> 0; 64 bits: a defective negative traj_idx does not overflow it)
        if (held == 0 && d <= (int64_t)k.detect && ((uint32_t)k.conflict[c.m] & occ) != 0) {
            const double v = a.state[4 * (size_t)q + 2];
            if (k.waited[q] != 0 || (double)d * a.dl >= v * v / (2.0 * a.sg.brake)) boxed = 1;
        }
        if (boxed != 0 && c.s < a.cut_len[q]) a.cut_len[q] = c.s;
        waited = held != 0 || boxed != 0 ? 1 : 0;
    }
    k.boxed[q] = boxed;
    k.waited[q] = waited;
    return boxed;
}

// the whole rule for junction j as one loop (the host's order; the kernel spreads the agents over a lane group); returns the agents boxed
MPCX_REC_FN int keepclear_junction(const KeepClearArgs &a, int j) {
    const mpcx_keepclear &k = a.kc;
    const int q0 = j * k.n_per;
    uint32_t occ = 0u;
    for (int m = 0; m < k.n_per; m++) occ |= keepclear_occupies(keepclear_classify(a.s, k, q0 + m));
    int got = 0;
    for (int m = 0; m < k.n_per; m++) got += keepclear_agent(a.s, k, q0 + m, keepclear_classify(a.s, k, q0 + m), occ);
    k.occupied[j] = (int32_t)occ;
    k.n_boxed[j] = got;
    return got;
}

}  // namespace mpcx
