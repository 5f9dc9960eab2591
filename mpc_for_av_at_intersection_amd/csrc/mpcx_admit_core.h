// mpcx_admit_core.h -- ADMISSION, the counterpart of departure: agents enter the scene on a schedule.  Host + device source (the pattern of
// mpcx_retire_core.h, mpcx_record_core.h and mpcx_traffic_core.h).  admit_snapshot_kernel and admit_gate_kernel (mpcx_admit.hip) run it as the
// FIRST two launches of a closed-loop step; tests/admit_ref/admit_ref.cpp builds it for the host.
//
// A scheduled agent WAITS in the state retirement and departure already know: done[q] = 1 and absent[own row] = 1.  It is not solved, not
// logged, not counted and not seen, and its buffers stay as they were allocated.  Per agent there is a word wait[q]:
//   -1    not scheduled, or already entered: the rule does not touch the agent
//   > 0   steps still to wait: decremented once per step, nothing else
//   0     DUE: the agent asks to enter in this step
// A due agent q is admitted in this step iff its start pose -- its state row, which never moved -- has clearance >= gap to every BLOCKING row
// of its pool window [obs_off, obs_off + obs_cnt) minus its own row.  A row blocks if
//   - it is present at the start of this step (absent[r] == 0, as the previous step left it), or
//   - it is the own row of another agent q' < q that is also due in this step -- whether or not q' itself gets in.
// The second clause is the tie-break: the outcome does not depend on the order in which lanes run, and two cars due at one pose never enter
// together.  The price: where q' is due and itself held back, q is judged against a car that does not appear, and may wait one step longer
// than strictly necessary.
// Clearance is the run log's: the two discs of either car (rec_discs of mpcx_record_core.h), hypot over the 2 x 2 pairs, minus 2 radius.
// The poses are those this step's pool WILL hold: an agent's is its state row; a scripted actor's is the row its get() emits in this step,
// obtained by traffic_get_step (mpcx_traffic_core.h) on a COPY of its four state doubles -- the stepped copy is thrown away, the actor's
// state is not written.  A pool row that is neither an agent's own row nor an actor's is nobody and never blocks.
// On admission: done[q] = 0, absent[own] = 0, wait[q] = -1, entered_step[q] = the clock as the step found it (closed-loop steps completed
// since admission was switched on; a device word, so a replayed graph counts like a plain run).
//
// Two passes, so that no lane reads a word another lane of the same launch writes (absent, done and wait are read AND written by the rule):
//   admit_snapshot_agent / admit_snapshot_actor   per pool row (x, y, yaw) and a tag -- ADMIT_GONE, ADMIT_PRESENT or ADMIT_DUE + q -- into a
//                         scratch table; reads state, absent, wait and the actors, writes only its own row of the table.
//                         admit_tick advances the clock (one lane).
//   admit_gate_agent      the gate for agent q from the table alone; reads wait[q] and the clock, writes wait[q], done[q], absent[own],
//                         entered_step[q] -- words of agent q only (agents' own rows are distinct).
// Every pool index is checked against the pool before it is read; an own row outside the pool is never admitted and never written.
#pragma once
#include "mpcx_record_core.h"
#include "mpcx_traffic_core.h"

namespace mpcx {

constexpr int32_t ADMIT_GONE = 0, ADMIT_PRESENT = 1, ADMIT_DUE = 2;     // tags of the table; ADMIT_DUE + q: absent, own row of the due agent q

struct AdmitArgs {
    int P, n_pool, n_actors;
    double radius, cc[4];           // mpcx_interaction_params.radius / circle_centers
    const double *state;            // P,4
    const int32_t *obs_off, *obs_cnt, *own_row;     // own_row: obs_skip
    int32_t *done, *absent;         // mpcx_retire::done (P), mpcx_scene::absent (n_pool)
    const mpcx_traffic_actor *actors;       // scripted traffic or n_actors = 0
    const double *actor_state, *tape;
    int64_t tape_rows;
    const int32_t *actor_row;
    mpcx_admit ad;
    double *tab_pose;               // n_pool,3: x, y, yaw
    int32_t *tab_tag;               // n_pool
};

MPCX_REC_FN void admit_snapshot_agent(const AdmitArgs &a, int q) {
    const int32_t own = a.own_row[q];
    if (own < 0 || own >= a.n_pool) return;
    const double *st = a.state + 4 * (size_t)q;
    double *p = a.tab_pose + 3 * (size_t)own;
    p[0] = st[0]; p[1] = st[1]; p[2] = st[3];
    a.tab_tag[own] = a.absent[own] == 0 ? ADMIT_PRESENT : (a.ad.wait[q] == 0 ? ADMIT_DUE + q : ADMIT_GONE);
}

// row6 (optional): the whole get() row, for the host build's comparison
MPCX_REC_FN void admit_snapshot_actor(const AdmitArgs &a, int i, double *row6 = nullptr) {
    const int32_t r = a.actor_row[i];
    if (r < 0 || r >= a.n_pool) return;
    const mpcx_traffic_actor act = a.actors[i];
    double st[4], row[6];
    for (int k = 0; k < 4; k++) st[k] = a.actor_state[4 * (size_t)i + k];
    traffic_get_step(act, st, a.tape, a.tape_rows, row);        // steps the copy; the actor's own state is traffic_kernel's to advance
    double *p = a.tab_pose + 3 * (size_t)r;
    p[0] = row[0]; p[1] = row[1]; p[2] = row[3];
    a.tab_tag[r] = a.absent[r] == 0 ? ADMIT_PRESENT : ADMIT_GONE;
    if (row6)
        for (int k = 0; k < 6; k++) row6[k] = row[k];
}

MPCX_REC_FN void admit_tick(const AdmitArgs &a) { *a.ad.clock += 1; }

// clearance of the poses p and o (x, y, yaw each)
MPCX_REC_FN double admit_pair_clearance(const AdmitArgs &a, const double *p, const double *o) {
    double ed[4], od[4];
    rec_discs(a.cc, p[0], p[1], p[2], ed);
    rec_discs(a.cc, o[0], o[1], o[2], od);
    double best = INFINITY;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            best = fmin(best, hypot(ed[2 * i] - od[2 * j], ed[2 * i + 1] - od[2 * j + 1]));
    return best - 2.0 * a.radius;
}

// The gate for agent q, AFTER the snapshot of this step (the clock has been advanced by it: the step found clock - 1).  Returns whether
// the agent was admitted.
MPCX_REC_FN bool admit_gate_agent(const AdmitArgs &a, int q) {
    const int32_t w = a.ad.wait[q];
    if (w != 0) {
        if (w > 0) a.ad.wait[q] = w - 1;
        return false;
    }
    const int32_t own = a.own_row[q];
    if (own < 0 || own >= a.n_pool) return false;
    const double *me = a.tab_pose + 3 * (size_t)own;
    int64_t lo = a.obs_off[q], hi = lo + (int64_t)a.obs_cnt[q];
    if (lo < 0) lo = 0;
    if (hi > a.n_pool) hi = a.n_pool;
    double clear = INFINITY;
    for (int64_t r = lo; r < hi; r++) {
        if (r == own) continue;
        const int32_t tag = a.tab_tag[r];
        const bool blocks = tag == ADMIT_PRESENT || (tag >= ADMIT_DUE && tag - ADMIT_DUE < q);
        if (blocks) clear = fmin(clear, admit_pair_clearance(a, me, a.tab_pose + 3 * (size_t)r));
    }
    if (!(clear >= a.ad.gap)) return false;
    a.done[q] = 0;
    a.absent[own] = 0;
    a.ad.wait[q] = -1;
    a.ad.entered_step[q] = *a.ad.clock - 1;
    return true;
}

}  // namespace mpcx
