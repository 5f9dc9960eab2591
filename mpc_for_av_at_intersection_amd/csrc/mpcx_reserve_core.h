// mpcx_reserve_core.h -- CROSSING RESERVATIONS: a manager per junction admits a car only if its MOVEMENT conflicts with no movement that
// holds the crossing; first come, first served, and cars wait at their stop lines.  Host + device source (the pattern of
// mpcx_actuated_core.h, whose hold it shares).  reserve_kernel (mpcx_reserve.hip) runs it with a lane group per junction in the place of
// signal_kernel / actuated_signal_kernel; tests/reserve_ref/reserve_ref.cpp builds it for the host.
//
// The movement of an agent is the signal group of its stop line (path_group, at most MPCX_SIGNAL_GROUPS_MAX).  A junction is n_per
// consecutive agents (n_per <= 64): junction j owns agents [j n_per, (j + 1) n_per).  Tables: path_exit[n_points] the route-local index e
// at which a vehicle on this point has left the crossing (-1: no crossing ahead or under the point); conflict[n_groups] bit h of word g =
// movements g and h may not hold the crossing together; lane[n_groups] bit h of word g = they queue in the same approach lane (bit g of
// word g is set); mgr_time[n_mgr][2] = (detect in path points, patience in steps); mgr_of[n_junctions].  State: grant[P] (0 / 1), since[P]
// (the clock value of the agent's first request, -1 = none), clock[n_junctions]; out: occupied[n_junctions], queued[n_junctions].
// Integers only.
//
// Per junction and step, in this order:
//   1. t = clock[j], a negative word counts as 0; clock[j] = t + 1 (wrapping into the negative words, which count as 0).  mgr_of[j] out of
//      range: no manager -- the agents are free (held = 0), grant, since and clock are left alone, occupied = queued = 0.
//   2. every agent q, with ti = traj_idx[q], i = path_off[q] + ti, s = path_stop[i], g = path_group[i], e = path_exit[i]:
//      OUT (grant = 0, since = -1): done[q] != 0; i outside [0, n_points); e < 0, e > path_len[q] or ti >= e; g outside [0, n_groups); or
//      ti < s with s >= path_len[q].  INSIDE (grant = 1, occupies g whatever grant was; since is left alone): not OUT and (s < 0 or
//      ti >= s).  APPROACH (ti < s): with grant != 0 it occupies g -- a grant is never revoked, grant and since are left alone --; without
//      a grant and with s - ti <= detect it REQUESTS, since = since >= 0 ? since : t; otherwise since = -1.
//   3. occ = OR of 1 << g over the occupying agents.
//   4. the requesters in ascending order of (since, min(s - ti, 65535), index within the junction), from ahead = blocked = 0: a requester
//      of movement g is granted (grant = 1, occ |= 1 << g) if (conflict[g] & (occ | blocked)) == 0 and (lane[g] & ahead) == 0; otherwise
//      it is denied, ahead |= 1 << g, and if it is aged, (int64) t - since >= patience, also blocked |= 1 << g.
//   5. occupied[j] = occ, queued[j] = the number denied.
//   6. every agent of the junction: signal_hold (mpcx_signal_core.h) -- an APPROACH agent sees GREEN with grant != 0 and RED otherwise,
//      everybody else is free.  There is no amber.
// The order of step 4 is one 64-bit key per requester, since << 32 | dist << 16 | index << 8 | g, and a loop of minima: the host walks an
// array, the kernel a lane group.  A junction's words are read before any of them is written, its agents' words are the agents' own: the
// outcome does not depend on the order of the junctions, nor on that of the lanes.
#pragma once
#include "mpcx_signal_core.h"

#define MPCX_RESERVE_OUT 0
#define MPCX_RESERVE_INSIDE 1
#define MPCX_RESERVE_APPROACH 2
#define MPCX_RESERVE_NO_KEY 0xffffffffffffffffull       /* the key of an agent that does not request */

namespace mpcx {

struct ReserveArgs {
    SignalArgs s;           // the hold's words: s.sg supplies path_stop, path_group, held, brake, n_points, n_groups
    mpcx_reservation rv;
};

struct ReserveAgent {
    int32_t kind, g, dist;  // MPCX_RESERVE_*; the movement (INSIDE, APPROACH); min(s - ti, 65535) (APPROACH)
    bool near;              // APPROACH: inside the detector
};

// the manager of junction j, -1 = none
MPCX_REC_FN int32_t reserve_mgr(const mpcx_reservation &r, int j) {
    const int32_t k = r.mgr_of[j];
    return k >= 0 && k < r.n_mgr ? k : -1;
}

// step 1: the clock as read
MPCX_REC_FN int32_t reserve_clock(int32_t word) { return word < 0 ? 0 : word; }
MPCX_REC_FN int32_t reserve_tick(int32_t t) { return (int32_t)((uint32_t)t + 1u); }

// step 2, the test: where agent q stands
MPCX_REC_FN ReserveAgent reserve_classify(const SignalArgs &a, const mpcx_reservation &r, int q, int32_t detect) {
    const mpcx_signals &sg = a.sg;
    ReserveAgent c{MPCX_RESERVE_OUT, 0, 0, false};
    if (a.done && a.done[q] != 0) return c;
    const int32_t ti = a.traj_idx[q];
    const int64_t i = (int64_t)a.path_off[q] + (int64_t)ti;
    if (i < 0 || i >= (int64_t)sg.n_points) return c;
    const int32_t s = sg.path_stop[i], g = sg.path_group[i], e = r.path_exit[i];
    if (e < 0 || e > a.path_len[q] || ti >= e || g < 0 || g >= sg.n_groups) return c;
    c.g = g;
    if (s < 0 || ti >= s) { c.kind = MPCX_RESERVE_INSIDE; return c; }
    if (s >= a.path_len[q]) return c;
    const int64_t d = (int64_t)s - (int64_t)ti;
    c.kind = MPCX_RESERVE_APPROACH;
    c.dist = d < 65535 ? (int32_t)d : 65535;
    c.near = d <= (int64_t)detect;
    return c;
}

// step 2, the words: grant and since of the agent at place idx of its junction as the step leaves them (before the grant loop), its bit in
// occ and its key, MPCX_RESERVE_NO_KEY unless it requests
struct ReserveWords {
    uint64_t key;
    int32_t grant, since;
    uint32_t occ;
};
MPCX_REC_FN ReserveWords reserve_request(const ReserveAgent &c, int32_t t, int idx, int32_t grant, int32_t since) {
    const uint32_t bit = 1u << c.g;
    if (c.kind == MPCX_RESERVE_OUT) return ReserveWords{MPCX_RESERVE_NO_KEY, 0, -1, 0u};
    if (c.kind == MPCX_RESERVE_INSIDE) return ReserveWords{MPCX_RESERVE_NO_KEY, 1, since, bit};
    if (grant != 0) return ReserveWords{MPCX_RESERVE_NO_KEY, grant, since, bit};
    if (!c.near) return ReserveWords{MPCX_RESERVE_NO_KEY, 0, -1, 0u};
    const int32_t first = since >= 0 ? since : t;
    const uint64_t key = (uint64_t)(uint32_t)first << 32 | (uint64_t)(uint32_t)c.dist << 16 | (uint64_t)(uint32_t)idx << 8 | (uint64_t)(uint32_t)c.g;
    return ReserveWords{key, 0, first, 0u};
}

// step 4: the masks of the grant loop, and the requester with the smallest key left decided on them; granted = the last decision
struct ReserveMasks {
    uint32_t occ, ahead, blocked;
    int32_t denied;
    bool granted;
};
MPCX_REC_FN ReserveMasks reserve_decide(const mpcx_reservation &r, uint64_t key, int32_t t, int32_t patience, ReserveMasks m) {
    const int32_t g = (int32_t)(key & 0xffu), since = (int32_t)(key >> 32);
    const uint32_t bit = 1u << g;
    m.granted = ((uint32_t)r.conflict[g] & (m.occ | m.blocked)) == 0 && ((uint32_t)r.lane[g] & m.ahead) == 0;
    if (m.granted) {
        m.occ |= bit;
    } else {
        m.ahead |= bit;
        m.denied += 1;
        if ((int64_t)t - (int64_t)since >= (int64_t)patience) m.blocked |= bit;
    }
    return m;
}

// the light of the hold: GREEN with a grant, RED without
struct GrantLight {
    int32_t grant;
    MPCX_REC_FN_MEMBER int operator()(int32_t) const { return grant != 0 ? MPCX_SIGNAL_GREEN : MPCX_SIGNAL_RED; }
};

// the whole rule for junction j as one loop (the host's order; the kernel spreads the agents over a lane group); returns the agents held
MPCX_REC_FN int reserve_junction(const ReserveArgs &a, int j) {
    const mpcx_reservation &r = a.rv;
    const int n = r.n_per < 64 ? r.n_per : 64;
    const int q0 = j * r.n_per;
    const int32_t k = reserve_mgr(r, j);
    int got = 0;
    if (k < 0) {
        r.occupied[j] = 0;
        r.queued[j] = 0;
        for (int q = q0; q < q0 + r.n_per; q++) got += signal_hold(a.s, q, false, GrantLight{0}) != 0 ? 1 : 0;
        return got;
    }
    const int32_t t = reserve_clock(r.clock[j]);
    const int32_t detect = r.mgr_time[2 * (size_t)k], patience = r.mgr_time[2 * (size_t)k + 1];
    r.clock[j] = reserve_tick(t);
    uint64_t key[64];
    bool approach[64];
    ReserveMasks mk{0u, 0u, 0u, 0, false};
    for (int m = 0; m < n; m++) {
        const ReserveAgent c = reserve_classify(a.s, r, q0 + m, detect);
        const ReserveWords w = reserve_request(c, t, m, r.grant[q0 + m], r.since[q0 + m]);
        approach[m] = c.kind == MPCX_RESERVE_APPROACH;
        key[m] = w.key;
        r.grant[q0 + m] = w.grant;
        r.since[q0 + m] = w.since;
        mk.occ |= w.occ;
    }
    for (;;) {
        int w = -1;
        for (int m = 0; m < n; m++)
            if (key[m] != MPCX_RESERVE_NO_KEY && (w < 0 || key[m] < key[w])) w = m;
        if (w < 0) break;
        mk = reserve_decide(r, key[w], t, patience, mk);
        if (mk.granted) r.grant[q0 + w] = 1;
        key[w] = MPCX_RESERVE_NO_KEY;
    }
    r.occupied[j] = (int32_t)mk.occ;
    r.queued[j] = mk.denied;
    for (int m = 0; m < n; m++) got += signal_hold(a.s, q0 + m, approach[m], GrantLight{r.grant[q0 + m]}) != 0 ? 1 : 0;
    return got;
}

}  // namespace mpcx
