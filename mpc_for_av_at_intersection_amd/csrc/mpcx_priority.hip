// mpcx_priority.hip -- priority road in the device-resident closed loop: the struct's checks and the stage that holds an agent of a minor
// movement at its stop line until the conflicting movements of smaller rank leave it a gap.  The rule is mpcx_priority_core.h.
// priority_kernel: one launch in the hold's place -- behind the conflict search and the safety stage, in front of the following stage --
// in both stop modes.  The layout is keepclear_kernel's: a LANE GROUP of G lanes per junction, G the smallest power of two >= n_per (n_per
// <= 64), one agent per lane, 64 / G junctions per wavefront (a block is one wavefront).  The pairing is ALL-TO-ALL, not a reduction: whom
// a lane counts depends on its own rank and conflict word.  Each lane classifies its agent and keeps (m, rank, eta); in G - 1 rounds every
// lane reads those of lane (sub + k) & (G - 1) of its group by __shfl -- the movement, the rank (any non-negative int32, so it does not
// share a word with the movement; an OUT agent and a padding lane carry the largest rank and pass nobody's filter) and the two halves of
// eta -- and keeps the lexicographic minimum of (eta, agent index) over what passes its filter, so the order of the rounds does not matter.
// One butterfly ORs the movements inside, one sums the agents yielding.  No lane leaves before the last shuffle: a dead group and a
// padding lane of a live group stay.  The group's first lane writes occupied and n_yielding, every lane its own words.  No lane reads a
// word another lane of the launch writes.  No LDS, no scratch, no atomics; rank, gap and conflict are read once per lane.  Everything it
// reads is device memory, so a replayed hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_priority_core.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mpcx {

template <int G>
__global__ __launch_bounds__(64) void priority_kernel(PriorityArgs a) {
    const mpcx_priority &k = a.pr;
    const int sub = threadIdx.x & (G - 1);
    const int j = blockIdx.x * (64 / G) + (threadIdx.x / G);
    const bool live = j < k.n_junctions;        // (a dead group stays for the shuffles: no lane leaves early)
    const bool mine = live && sub < k.n_per;    // (so does a padding lane of a live group)
    const int q0 = live ? j * k.n_per : 0;
    const int q = mine ? q0 + sub : 0;
    PriorityAgent me{MPCX_KEEPCLEAR_OUT, 0, INT32_MAX, 0, 0, 0u, 0.0};
    if (mine) me = priority_classify(a, q);
    const int eta_lo = __double2loint(me.eta), eta_hi = __double2hiint(me.eta);
    double lag = INFINITY;
    int32_t blocker = -1;
#pragma unroll
    for (int r = 1; r < G; r++) {
        const int from = (sub + r) & (G - 1);
        const int32_t m_r = __shfl(me.m, from, G), rank_r = __shfl(me.rank, from, G);
        const double eta_r = __hiloint2double(__shfl(eta_hi, from, G), __shfl(eta_lo, from, G));
        priority_meet(me, m_r, rank_r, eta_r, q0 + from, lag, blocker);
    }
    uint32_t occ = priority_occupies(me);
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) occ |= (uint32_t)__shfl_xor((int)occ, m, G);
    int32_t n = mine ? priority_agent(a, q, me, lag, blocker) : 0;
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, G);
    if (live && sub == 0) {
        k.occupied[j] = (int32_t)occ;
        k.n_yielding[j] = n;
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no priority stage"
bool mpcx_priority_absent(const mpcx_priority *s) {
    if (!s) return true;
    mpcx_priority z;
    memset(&z, 0, sizeof z);
    return memcmp(s, &z, sizeof z) == 0;        // (the struct has no padding)
}
static_assert(sizeof(mpcx_priority) == 136, "mpcx_priority has padding: mpcx_priority_absent and the cached graph's key compare its bytes");

// the struct's own fields and what the stage needs of the run.  exchange: the descriptor's (0 for a stage call); held_run: the run carries
// signals, actuation or a reservation.  Never a GPU fault for a bad struct.  The three per-movement tables are read back (blocking copies,
// never inside a capture) ONCE per struct: ctx->priority_tables remembers the pointers and count that passed, and mpcx_set_priority forgets
// them when the struct it is given differs from the one it holds -- so a run(1) in a loop checks nothing again.
int32_t mpcx_priority_validate(mpcx_ctx *ctx, const mpcx_priority *s, int32_t P, int32_t exchange, bool held_run) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: null struct");
    if (held_run)
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: the run also carries signals, actuation or a reservation (a junction is run by lights, by a manager, or by priority)");
    const char *missing = !s->path_stop ? "path_stop" : !s->path_move ? "path_move" : !s->path_exit ? "path_exit" : !s->conflict ? "conflict" :
                          !s->rank ? "rank" : !s->gap ? "gap" : !s->waited ? "waited" : !s->yielding ? "yielding" : !s->blocker ? "blocker" :
                          !s->lag ? "lag" : !s->occupied ? "occupied" : !s->n_yielding ? "n_yielding" : nullptr;
    if (missing) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: %s is null (all twelve pointers are required)", missing);
    if (s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: the reserved word is not 0");
    if (s->n_per < 1 || s->n_per > MPCX_PRIORITY_PER_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: n_per = %d outside 1..%d", s->n_per, MPCX_PRIORITY_PER_MAX);
    if (s->n_junctions < 0 || (int64_t)s->n_per * (int64_t)s->n_junctions != (int64_t)P)
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: n_per * n_junctions = %d * %d is not P = %d", s->n_per, s->n_junctions, P);
    if (s->n_moves < 1 || s->n_moves > MPCX_SIGNAL_GROUPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: n_moves = %d outside 1..%d", s->n_moves, MPCX_SIGNAL_GROUPS_MAX);
    if (s->n_points < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: n_points = %d (at least 1 path point)", s->n_points);
    if (s->detect < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: detect = %d (at least 1 path point)", s->detect);
    if (!std::isfinite(s->v_floor) || !(s->v_floor > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: v_floor = %g must be finite and positive", s->v_floor);
    if (!std::isfinite(s->brake) || !(s->brake > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: brake = %g must be finite and positive", s->brake);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: not supported in the agent-sharded layout (shard by instances)");
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority: %d linearisation passes; the stage sits in front of a single window stage", ctx->lin_passes);
    mpcx_ctx::PriorityTables &t = ctx->priority_tables;
    if (t.ok && t.conflict == s->conflict && t.rank == s->rank && t.gap == s->gap && t.n_moves == s->n_moves) return MPCX_OK;
    t.ok = false;
    const size_t nm = (size_t)s->n_moves;
    std::vector<int32_t> cf(nm), rk(nm);
    std::vector<double> gp(nm);
    if (hipMemcpy(cf.data(), s->conflict, nm * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rk.data(), s->rank, nm * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(gp.data(), s->gap, nm * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "priority: cannot read the conflict, rank and gap tables back for their check");
    const uint32_t all = (1u << s->n_moves) - 1u;
    for (size_t g = 0; g < nm; g++) {
        const uint32_t c = (uint32_t)cf[g];
        if ((c & ~all) != 0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "priority: movement %d has conflict = 0x%x with bits at or above n_moves = %d", (int)g, c, s->n_moves);
        if ((c >> g) & 1u) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: movement %d conflicts with itself (conflict = 0x%x)", (int)g, c);
        for (size_t h = 0; h < nm; h++)
            if (((c >> h) & 1u) != (((uint32_t)cf[h] >> g) & 1u))
                return mpcx_fail(ctx, MPCX_E_INVALID, "priority: conflict is not symmetric at movements %d and %d", (int)g, (int)h);
        if (rk[g] < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "priority: movement %d has the negative rank %d", (int)g, rk[g]);
        if (!std::isfinite(gp[g]) || gp[g] < 0.0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "priority: movement %d has gap = %g (finite and not negative)", (int)g, gp[g]);
    }
    t.conflict = s->conflict; t.rank = s->rank; t.gap = s->gap; t.n_moves = s->n_moves; t.ok = true;
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_priority(mpcx_ctx *ctx, const mpcx_priority *s) {
    if (!ctx) return MPCX_E_INVALID;
    mpcx_priority f;
    memset(&f, 0, sizeof f);
    const bool have = !mpcx_priority_absent(s);
    if (have) f = *s;                                           // (no padding: the cached graph's key takes the struct as it stands)
    if (have != ctx->have_priority || memcmp(&f, &ctx->priority, sizeof f) != 0) ctx->priority_tables.ok = false;    // a new struct: its tables are checked again
    memcpy(&ctx->priority, &f, sizeof f);
    ctx->have_priority = have;
    return MPCX_OK;
}

// the launch alone (the struct has been checked): what the closed loop enqueues in the hold's place, also inside a capture
int32_t mpcx_priority_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                              const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const mpcx_priority *priority) {
    mpcx::PriorityArgs a;
    memset(&a, 0, sizeof a);
    mpcx_signals sg;
    memset(&sg, 0, sizeof sg);
    sg.path_stop = priority->path_stop;         // (the classification reads the stop line where the signals keep it)
    a.s = mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg};
    a.pr = *priority;
    const int J = priority->n_junctions, n = priority->n_per;
    if (J == 0) return MPCX_OK;
#define MPCX_PR_LAUNCH(G) hipLaunchKernelGGL(mpcx::priority_kernel<G>, dim3((J + 64 / G - 1) / (64 / G)), dim3(64), 0, ctx->stream, a)
    if (n <= 1) MPCX_PR_LAUNCH(1);
    else if (n <= 2) MPCX_PR_LAUNCH(2);
    else if (n <= 4) MPCX_PR_LAUNCH(4);
    else if (n <= 8) MPCX_PR_LAUNCH(8);
    else if (n <= 16) MPCX_PR_LAUNCH(16);
    else if (n <= 32) MPCX_PR_LAUNCH(32);
    else MPCX_PR_LAUNCH(64);
#undef MPCX_PR_LAUNCH
    return mpcx_check_launch(ctx, "priority_kernel");
}

extern "C" int32_t mpcx_priority_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off,
                                            const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                                            const mpcx_priority *priority) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "priority_step_batch: negative size");
    ctx->priority_tables.ok = false;        // (the struct is the argument's: its tables are read back in every stage call)
    const int32_t rc = mpcx_priority_validate(ctx, priority, P, 0, false);
    ctx->priority_tables.ok = false;
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !path_len || !traj_idx || !cut_len || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "priority_step_batch: null buffer (state, path_off, path_len, traj_idx, cut_len) or dl <= 0");
    return mpcx_priority_enqueue(ctx, P, dl, state, path_off, path_len, traj_idx, cut_len, done, priority);
}
