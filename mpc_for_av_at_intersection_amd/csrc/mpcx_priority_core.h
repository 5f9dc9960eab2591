// mpcx_priority_core.h -- PRIORITY ROAD: an agent of a minor movement waits at its stop line until the conflicting movements of smaller rank
// leave it a gap.  Host + device source (the pattern of mpcx_keepclear_core.h, whose classification it calls).  priority_kernel
// (mpcx_priority.hip) runs it with a lane group per junction in the hold's place -- behind the conflict search and the safety stage, in
// front of the following stage; tests/priority_ref/priority_ref.cpp builds it for the host.
//
// There are no signals in the run: the stop line, the movement and the exit point of a path point are the stage's own tables.  A junction is
// n_per consecutive agents (n_per <= 64): junction j owns agents [j n_per, (j + 1) n_per).  Tables: path_stop[n_points], path_move[n_points],
// path_exit[n_points] as the signals' and keep clear's; conflict[n_moves] bit h of word g = movements g and h cross (symmetric, no self-bit);
// rank[n_moves] >= 0, a smaller rank goes first; gap[n_moves] the critical gap in seconds of movement m when it gives way.  Scalars: v_floor
// (> 0, the speed an approaching car is taken to have at least), brake (> 0), detect (>= 1 path point).  State: waited[P] in-out,
// zero-initialised; out: yielding[P] (0 / 1), blocker[P] (an agent index, -1 = none), lag[P] (seconds, +inf = none), occupied[n_junctions],
// n_yielding[n_junctions].
//
// Per junction and step, everything is read before anything is written:
//   1. every agent q is OUT, INSIDE or APPROACH with (m, s, ti) as keepclear_classify decides, path_stop being the stage's own.
//   2. an agent r that is not OUT has eta_r = 0.0 if INSIDE, else (double)(s_r - ti_r) * dl / fmax(state[r][2], v_floor): one multiply and
//      one divide.  occ = OR of 1 << m over the INSIDE agents.
//   3. an APPROACH agent q with s_q - ti_q <= detect is a CANDIDATE: lag[q] = the minimum of eta_r over the agents r != q of the junction
//      that are not OUT, have rank[m_r] < rank[m_q] and bit m_r of conflict[m_q] set; blocker[q] = the agent that attains it, the lowest
//      index among equals; none: +inf and -1.  q is THREATENED iff lag[q] < gap[m_q].  Everybody else: lag = +inf, blocker = -1, yielding =
//      0, waited = 0.
//   4. a threatened q YIELDS if waited[q] != 0 or if it can still stop, (double)(s - ti) * dl >= v * v / (2.0 * brake) -- signal_hold's
//      expression; otherwise it is free and left to the conflict search, as on amber.  Yields: yielding[q] = 1, cut_len[q] = min(cut_len[q], s).
//   5. waited[q] = yielding[q].
//   6. occupied[j] = occ, n_yielding[j] = the number yielding.
// The minimum is the lexicographic minimum of (eta, agent index) over what passes q's filter, so it does not depend on the order in which
// the others are visited: the host walks the junction, the kernel rotates through its lane group.  eta is an IEEE division, the rest
// comparisons; nothing can fuse, host builds use -ffp-contract=off all the same.  A NaN speed counts as v_floor (fmax).
//
// What the order implies: cut_len is only lowered, so a conflict cut in front of the line is kept; the stage writes no word of another
// stage.  A vehicle that arrives has been OUT since its exit point and a slot reset by the respawn stage is OUT while it waits at the gate
// (done[q] != 0), so step 3 has cleared its waited word before the next vehicle drives: the word heals itself.  The outcome depends neither
// on the order of the junctions nor on that of the lanes, and a replayed hipGraph counts like a plain run.
#pragma once
#include "mpcx_keepclear_core.h"
#include <cmath>
#include <cstdint>

namespace mpcx {

struct PriorityArgs {
    SignalArgs s;           // the hold's words; of s.sg only path_stop is set (the stage's own table): what keepclear_classify reads
    mpcx_priority pr;
};

struct PriorityAgent {
    int32_t kind, m, rank;  // MPCX_KEEPCLEAR_*; the movement and its rank (INSIDE, APPROACH; an OUT agent carries the largest rank: it
                            // passes nobody's filter)
    int64_t d;              // s - ti, path points to the line (APPROACH; 64 bits: a defective negative traj_idx does not overflow it)
    int32_t s;              // the line (APPROACH)
    uint32_t cf;            // conflict[m] (INSIDE, APPROACH)
    double eta;             // seconds to the line at the present speed, 0.0 inside
};

// step 2: seconds to the line of an APPROACH agent d path points before it at speed v (also what a stop-sign junction sees of an unsigned car)
MPCX_REC_FN double priority_eta(int64_t d, double dl, double v, double v_floor) { return (double)d * dl / fmax(v, v_floor); }

// steps 1 and 2 for agent q: keepclear_classify on the stage's own tables, then the movement's rank and conflict word and the agent's eta
MPCX_REC_FN PriorityAgent priority_classify(const PriorityArgs &a, int q) {
    const mpcx_priority &k = a.pr;
    const mpcx_keepclear view{k.path_move, k.path_exit, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, k.n_moves, k.n_points, 0};
    const KeepClearAgent c = keepclear_classify(a.s, view, q);
    PriorityAgent p{c.kind, c.m, INT32_MAX, 0, c.s, 0u, 0.0};
    if (c.kind == MPCX_KEEPCLEAR_OUT) return p;
    p.rank = k.rank[c.m];
    p.cf = (uint32_t)k.conflict[c.m];
    if (c.kind == MPCX_KEEPCLEAR_APPROACH) {
        p.d = (int64_t)c.s - (int64_t)c.ti;
        p.eta = priority_eta(p.d, a.s.dl, a.s.state[4 * (size_t)q + 2], k.v_floor);
    }
    return p;
}

// step 2: the agent's bit in occ
MPCX_REC_FN uint32_t priority_occupies(const PriorityAgent &p) { return p.kind == MPCX_KEEPCLEAR_INSIDE ? 1u << p.m : 0u; }

// step 3, one other agent r (movement m_r of rank rank_r, eta_r; r != q) seen by agent q: keeps the lexicographic minimum of (eta, index)
// over what passes q's filter in (lag, blocker), which start as (+inf, -1)
MPCX_REC_FN void priority_meet(const PriorityAgent &me, int32_t m_r, int32_t rank_r, double eta_r, int32_t r, double &lag, int32_t &blocker) {
    if (rank_r < me.rank && ((me.cf >> m_r) & 1u) != 0 && (eta_r < lag || (eta_r == lag && (blocker < 0 || r < blocker)))) {
        lag = eta_r;
        blocker = r;
    }
}

// steps 3 - 5 for agent q on what it met: writes lag[q], blocker[q], yielding[q] and waited[q], lowers cut_len[q]; returns yielding[q]
MPCX_REC_FN int32_t priority_agent(const PriorityArgs &a, int q, const PriorityAgent &me, double lag, int32_t blocker) {
    const mpcx_priority &k = a.pr;
    const bool candidate = me.kind == MPCX_KEEPCLEAR_APPROACH && me.d <= (int64_t)k.detect;
    int32_t yielding = 0;
    if (!candidate) {
        lag = INFINITY;
        blocker = -1;
    } else if (lag < k.gap[me.m]) {
        const double v = a.s.state[4 * (size_t)q + 2];
        if (k.waited[q] != 0 || (double)me.d * a.s.dl >= v * v / (2.0 * k.brake)) yielding = 1;
        if (yielding != 0 && me.s < a.s.cut_len[q]) a.s.cut_len[q] = me.s;
    }
    k.lag[q] = lag;
    k.blocker[q] = blocker;
    k.yielding[q] = yielding;
    k.waited[q] = yielding;
    return yielding;
}

// the whole rule for junction j as loops (the host's order; the kernel spreads the agents over a lane group); returns the agents yielding
MPCX_REC_FN int priority_junction(const PriorityArgs &a, int j) {
    const mpcx_priority &k = a.pr;
    const int q0 = j * k.n_per;
    PriorityAgent ag[MPCX_PRIORITY_PER_MAX];
    uint32_t occ = 0u;
    for (int m = 0; m < k.n_per; m++) {
        ag[m] = priority_classify(a, q0 + m);
        occ |= priority_occupies(ag[m]);
    }
    int got = 0;
    for (int m = 0; m < k.n_per; m++) {
        double lag = INFINITY;
        int32_t blocker = -1;
        for (int r = 0; r < k.n_per; r++)
            if (r != m) priority_meet(ag[m], ag[r].m, ag[r].rank, ag[r].eta, q0 + r, lag, blocker);
        got += priority_agent(a, q0 + m, ag[m], lag, blocker);
    }
    k.occupied[j] = (int32_t)occ;
    k.n_yielding[j] = got;
    return got;
}

}  // namespace mpcx
