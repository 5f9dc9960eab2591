// mpcx_precedence_core.h -- RIGHT OF WAY BY ORDER OF ENTRY: the stamp of MPCX_PRECEDENCE_ENTRY.  Host + device source (the pattern of
// mpcx_admit_core.h and mpcx_route_core.h).  precedence_stamp_kernel (mpcx_precedence.hip) runs it one lane per agent right after the
// admission stage of a closed-loop step; tests/precedence_ref/precedence_ref.cpp builds it for the host.
//
// One int32 word per pool row, prec[n_rows], a smaller word goes first (mpcx_precedence in include/mpcx.h has the rule the conflict search
// applies to the words).  First come, first served: for every agent q that is in the scene -- entered_step[q] >= 0, the clock value the
// admission gate wrote when it let q in, 0 for an agent present from the start -- whose own row o = own_row[q] lies inside the pool,
//   prec[o] = entered_step[q] * 64 + (o - obs_off[q])
// i.e. the step of entry, ties to the lower window offset (a scene window holds at most 64 rows, MPCX_PRECEDENCE_WINDOW).  A waiting agent
// (entered_step[q] < 0) writes nothing: its row is absent and nobody looks at its word; it gets its word in the step that admits it, before
// that step's conflict search, and so queues behind everybody already in the scene.  Rows that are nobody's own -- scripted actors, unused
// rows -- keep the word the caller gave them.  The word of an agent does not change while it is in the scene: the stamp rewrites the same
// value every step, and the launch needs no knowledge of who was admitted just now.
// Every lane writes one word of its own agent's row (agents' own rows are distinct) and reads nothing another lane writes, so the outcome
// does not depend on the order of the lanes.  entered_step * 64 overflows int32 from step 2^25 on (about 78 days of simulated time at
// dt = 0.2 s): the product is formed in unsigned arithmetic, so it wraps without undefined behaviour, and the order is then wrong -- the
// caller's limit, MPCX_PRECEDENCE_MAX_STEP; the Python package refuses to run that far.
#pragma once
#include "mpcx_record_core.h"

#define MPCX_PRECEDENCE_WINDOW 64
#define MPCX_PRECEDENCE_MAX_STEP ((0x7fffffff - (MPCX_PRECEDENCE_WINDOW - 1)) / MPCX_PRECEDENCE_WINDOW)   /* the largest entered_step whose word fits */

namespace mpcx {

struct StampArgs {
    int P, n_rows;
    const int32_t *obs_off, *own_row;       // own_row: obs_skip
    const int32_t *entered_step;            // mpcx_admit::entered_step
    int32_t *prec;                          // mpcx_precedence::prec, n_rows words
};

// returns whether a word was written
MPCX_REC_FN bool precedence_stamp_agent(const StampArgs &a, int q) {
    const int32_t e = a.entered_step[q];
    if (e < 0) return false;                // waiting (or never scheduled and never in)
    const int32_t o = a.own_row[q];
    if (o < 0 || o >= a.n_rows) return false;       // (checked by the host; never written outside the pool)
    a.prec[o] = (int32_t)((uint32_t)e * (uint32_t)MPCX_PRECEDENCE_WINDOW + (uint32_t)(o - a.obs_off[q]));
    return true;
}

}  // namespace mpcx
