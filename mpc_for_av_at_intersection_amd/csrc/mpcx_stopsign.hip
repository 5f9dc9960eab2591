// mpcx_stopsign.hip -- stop signs in the device-resident closed loop: the struct's checks and the stage that holds an agent of a signed
// movement at its stop line until it has stood there and its turn has come.  The rule is mpcx_stopsign_core.h.
// stopsign_kernel: one launch in the hold's place -- behind the conflict search and the safety stage, in front of the following stage,
// where priority_kernel runs -- in both stop modes.  The layout is priority_kernel's: a LANE GROUP of G lanes per junction, G the smallest
// power of two >= n_per (n_per <= 64), one agent per lane, 64 / G junctions per wavefront (a block is one wavefront).  Each lane classifies
// its agent and keeps its words in registers; one butterfly ORs the occupied movements.  The lag is an ALL-TO-ALL pairing: in G - 1 rounds
// every lane reads of lane (sub + k) & (G - 1) of its group by __shfl the movement of an unsigned approaching agent (-1 for everybody
// else, padding lanes included) and the two halves of its eta, and keeps the lexicographic minimum of (eta, agent index) over what crosses
// its own movement, so the order of the rounds does not matter.  The release order is a loop of group-wide minima over one 64-bit key per
// requester (stopped_at << 32 | lane << 16 | (lag >= gap) << 8 | movement, all ones for a lane that does not request), a butterfly on the
// key's two halves: every lane of the group evaluates the winner's test on uniform words (conflict[m] and lane[m] are one load each, the
// same address in the whole group), so occ, ahead and blocked stay uniform across the group; the winning lane takes the result and retires
// its key.  A round serves one requester of every junction of the wavefront; the loop ends when no group of the wavefront has a requester
// left (one ballot per round), after at most n_per rounds.  One butterfly sums the agents waiting and one those that ran the sign.  No
// lane leaves before the last shuffle: a dead group and a padding lane of a live group stay.  The group's first lane writes clock, ran,
// occupied and n_waiting with plain stores, every lane its own words.  All lanes of a group sit in one wavefront and every read of a word
// stands before its write in program order, so no lane reads a word another lane of the launch writes.  No LDS, no scratch, no atomics.
// Everything it reads is device memory, so a replayed hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_stopsign_core.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mpcx {

// the minimum of a 64-bit key over the lane group
template <int G>
__device__ __forceinline__ uint64_t stopsign_min_key(uint64_t key) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, m, G), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), m, G);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        key = other < key ? other : key;
    }
    return key;
}

template <int G>
__global__ __launch_bounds__(64) void stopsign_kernel(StopSignArgs a) {
    const mpcx_stopsign &k = a.ss;
    const int sub = threadIdx.x & (G - 1);
    const int j = blockIdx.x * (64 / G) + (threadIdx.x / G);
    const bool live = j < k.n_junctions;        // (a dead group stays for the shuffles: no lane leaves early)
    const bool mine = live && sub < k.n_per;    // (so does a padding lane of a live group)
    const int q0 = live ? j * k.n_per : 0;
    const int q = mine ? q0 + sub : 0;
    const int32_t t = live ? reserve_clock(k.clock[j]) : 0;
    StopSignAgent me{0, 0, -1, 0, -1, 0, 0, 0u, 0u, 0, 0.0};
    if (mine) me = stopsign_classify(a, q, t);
    StopSignMasks mk{me.occ, 0u, 0u, false};
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) mk.occ |= (uint32_t)__shfl_xor((int)mk.occ, m, G);
    const int eta_lo = __double2loint(me.eta), eta_hi = __double2hiint(me.eta);
    double lag = INFINITY;
    int32_t blocker = -1;
#pragma unroll
    for (int r = 1; r < G; r++) {
        const int from = (sub + r) & (G - 1);
        const int32_t um_r = __shfl(me.um, from, G);
        const double eta_r = __hiloint2double(__shfl(eta_hi, from, G), __shfl(eta_lo, from, G));
        stopsign_meet(me, um_r, eta_r, q0 + from, lag, blocker);
    }
    uint64_t key = mine ? stopsign_key(k, me, sub, lag) : MPCX_STOPSIGN_NO_KEY;
    for (;;) {
        const uint64_t first = stopsign_min_key<G>(key);
        const bool any = first != MPCX_STOPSIGN_NO_KEY;
        if (__ballot(any) == 0) break;          // wavefront-uniform: every lane has taken part in this round's shuffles
        if (any) {
            mk = stopsign_decide(k, first, t, mk);
            if (key == first) {                 // (the lane index is part of the key: one lane of the group)
                if (mk.released) me.go = 1;
                key = MPCX_STOPSIGN_NO_KEY;
            }
        }
    }
    int32_t n = mine ? stopsign_agent(a, q, me, lag, blocker) : 0;
    int32_t ran = me.ran;
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        n += __shfl_xor(n, m, G);
        ran += __shfl_xor(ran, m, G);
    }
    if (live && sub == 0) {
        k.clock[j] = reserve_tick(t);
        k.ran[j] = (int32_t)((uint32_t)k.ran[j] + (uint32_t)ran);
        k.occupied[j] = (int32_t)mk.occ;
        k.n_waiting[j] = n;
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no stop-sign stage"
bool mpcx_stopsign_absent(const mpcx_stopsign *s) {
    if (!s) return true;
    mpcx_stopsign z;
    memset(&z, 0, sizeof z);
    return memcmp(s, &z, sizeof z) == 0;        // (the struct has no padding)
}
static_assert(sizeof(mpcx_stopsign) == 184, "mpcx_stopsign has padding: mpcx_stopsign_absent and the cached graph's key compare its bytes");

// the struct's own fields and what the stage needs of the run.  exchange: the descriptor's (0 for a stage call); other: what else runs the
// junction in this run (signals, actuation, a reservation: "lights or a manager"; the priority road), nullptr = nothing.  Never a GPU fault
// for a bad struct.  The four per-movement tables are read back (blocking copies, never inside a capture) ONCE per struct:
// ctx->stopsign_tables remembers the pointers and count that passed, and mpcx_set_stopsign forgets them when the struct it is given
// differs from the one it holds -- so a run(1) in a loop checks nothing again.
int32_t mpcx_stopsign_validate(mpcx_ctx *ctx, const mpcx_stopsign *s, int32_t P, int32_t exchange, const char *other) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: null struct");
    if (other)
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: the run also carries %s (a junction is run by lights, by a manager, by priority, or by signs)", other);
    const char *missing = !s->path_stop ? "path_stop" : !s->path_move ? "path_move" : !s->path_exit ? "path_exit" : !s->conflict ? "conflict" :
                          !s->lane ? "lane" : !s->sign ? "sign" : !s->gap ? "gap" : !s->stopped_at ? "stopped_at" : !s->go ? "go" :
                          !s->stopping ? "stopping" : !s->clock ? "clock" : !s->ran ? "ran" : !s->lag ? "lag" : !s->blocker ? "blocker" :
                          !s->occupied ? "occupied" : !s->n_waiting ? "n_waiting" : nullptr;
    if (missing) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: %s is null (all sixteen pointers are required)", missing);
    if (s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: the reserved word is not 0");
    if (s->n_per < 1 || s->n_per > MPCX_STOPSIGN_PER_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: n_per = %d outside 1..%d", s->n_per, MPCX_STOPSIGN_PER_MAX);
    if (s->n_junctions < 0 || (int64_t)s->n_per * (int64_t)s->n_junctions != (int64_t)P)
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: n_per * n_junctions = %d * %d is not P = %d", s->n_per, s->n_junctions, P);
    if (s->n_moves < 1 || s->n_moves > MPCX_SIGNAL_GROUPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: n_moves = %d outside 1..%d", s->n_moves, MPCX_SIGNAL_GROUPS_MAX);
    if (s->n_points < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: n_points = %d (at least 1 path point)", s->n_points);
    if (s->zone < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: zone = %d (at least 1 path point)", s->zone);
    if (s->zone > s->detect) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: zone = %d exceeds detect = %d", s->zone, s->detect);
    if (s->patience < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: patience = %d is negative", s->patience);
    if (!std::isfinite(s->v_stop) || !(s->v_stop > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: v_stop = %g must be finite and positive", s->v_stop);
    if (!std::isfinite(s->brake) || !(s->brake > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: brake = %g must be finite and positive", s->brake);
    if (!std::isfinite(s->v_floor) || !(s->v_floor > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: v_floor = %g must be finite and positive", s->v_floor);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: not supported in the agent-sharded layout (shard by instances)");
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: %d linearisation passes; the stage sits in front of a single window stage", ctx->lin_passes);
    mpcx_ctx::StopSignTables &t = ctx->stopsign_tables;
    if (t.ok && t.conflict == s->conflict && t.lane == s->lane && t.sign == s->sign && t.gap == s->gap && t.n_moves == s->n_moves) return MPCX_OK;
    t.ok = false;
    const size_t nm = (size_t)s->n_moves;
    std::vector<int32_t> cf(nm), ln(nm), sn(nm);
    std::vector<double> gp(nm);
    if (hipMemcpy(cf.data(), s->conflict, nm * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ln.data(), s->lane, nm * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(sn.data(), s->sign, nm * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(gp.data(), s->gap, nm * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "stopsign: cannot read the conflict, lane, sign and gap tables back for their check");
    const uint32_t all = (uint32_t)((1ull << s->n_moves) - 1ull);
    for (size_t g = 0; g < nm; g++) {
        const uint32_t c = (uint32_t)cf[g], l = (uint32_t)ln[g];
        if ((c & ~all) != 0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: movement %d has conflict = 0x%x with bits at or above n_moves = %d", (int)g, c, s->n_moves);
        if ((c >> g) & 1u) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: movement %d conflicts with itself (conflict = 0x%x)", (int)g, c);
        for (size_t h = 0; h < nm; h++)
            if (((c >> h) & 1u) != (((uint32_t)cf[h] >> g) & 1u))
                return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: conflict is not symmetric at movements %d and %d", (int)g, (int)h);
        if ((l & ~all) != 0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: movement %d has lane = 0x%x with bits at or above n_moves = %d", (int)g, l, s->n_moves);
        if (((l >> g) & 1u) == 0) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: movement %d is not in its own lane (lane = 0x%x)", (int)g, l);
        if (sn[g] != 0 && sn[g] != 1) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: movement %d has sign = %d (0 or 1)", (int)g, sn[g]);
        if (!std::isfinite(gp[g]) || gp[g] < 0.0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign: movement %d has gap = %g (finite and not negative)", (int)g, gp[g]);
    }
    t.conflict = s->conflict; t.lane = s->lane; t.sign = s->sign; t.gap = s->gap; t.n_moves = s->n_moves; t.ok = true;
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_stopsign(mpcx_ctx *ctx, const mpcx_stopsign *s) {
    if (!ctx) return MPCX_E_INVALID;
    mpcx_stopsign f;
    memset(&f, 0, sizeof f);
    const bool have = !mpcx_stopsign_absent(s);
    if (have) f = *s;                                           // (no padding: the cached graph's key takes the struct as it stands)
    if (have != ctx->have_stopsign || memcmp(&f, &ctx->stopsign, sizeof f) != 0) ctx->stopsign_tables.ok = false;    // a new struct: its tables are checked again
    memcpy(&ctx->stopsign, &f, sizeof f);
    ctx->have_stopsign = have;
    return MPCX_OK;
}

// the launch alone (the struct has been checked): what the closed loop enqueues in the hold's place, also inside a capture
int32_t mpcx_stopsign_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                              const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const mpcx_stopsign *stopsign) {
    mpcx::StopSignArgs a;
    memset(&a, 0, sizeof a);
    mpcx_signals sg;
    memset(&sg, 0, sizeof sg);
    sg.path_stop = stopsign->path_stop;         // (the classification reads the stop line where the signals keep it)
    a.s = mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg};
    a.ss = *stopsign;
    const int J = stopsign->n_junctions, n = stopsign->n_per;
    if (J == 0) return MPCX_OK;
#define MPCX_SS_LAUNCH(G) hipLaunchKernelGGL(mpcx::stopsign_kernel<G>, dim3((J + 64 / G - 1) / (64 / G)), dim3(64), 0, ctx->stream, a)
    if (n <= 1) MPCX_SS_LAUNCH(1);
    else if (n <= 2) MPCX_SS_LAUNCH(2);
    else if (n <= 4) MPCX_SS_LAUNCH(4);
    else if (n <= 8) MPCX_SS_LAUNCH(8);
    else if (n <= 16) MPCX_SS_LAUNCH(16);
    else if (n <= 32) MPCX_SS_LAUNCH(32);
    else MPCX_SS_LAUNCH(64);
#undef MPCX_SS_LAUNCH
    return mpcx_check_launch(ctx, "stopsign_kernel");
}

extern "C" int32_t mpcx_stopsign_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off,
                                            const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                                            const mpcx_stopsign *stopsign) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign_step_batch: negative size");
    ctx->stopsign_tables.ok = false;        // (the struct is the argument's: its tables are read back in every stage call)
    const int32_t rc = mpcx_stopsign_validate(ctx, stopsign, P, 0, nullptr);
    ctx->stopsign_tables.ok = false;
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !path_len || !traj_idx || !cut_len || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "stopsign_step_batch: null buffer (state, path_off, path_len, traj_idx, cut_len) or dl <= 0");
    return mpcx_stopsign_enqueue(ctx, P, dl, state, path_off, path_len, traj_idx, cut_len, done, stopsign);
}
