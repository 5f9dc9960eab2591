// mpcx_reserve.hip -- crossing reservations in the device-resident closed loop: the struct's checks and the stage that runs a manager per
// junction and holds the junction's agents at their stop lines.  The rule is mpcx_reserve_core.h; the hold is mpcx_signal_core.h's.
// reserve_kernel: one launch in the place of signal_kernel / actuated_signal_kernel, directly after the conflict search and before the
// window stage, in both stop modes.  A LANE GROUP of G lanes per junction, G the smallest power of two >= n_per (n_per <= 64), one agent
// per lane, 64 / G junctions per wavefront (a block is one wavefront).  Each lane classifies its agent and updates its grant and since in
// registers; a butterfly of __shfl_xor within the group ORs the occupied movements.  The ordered grant is a loop of group-wide minima over
// one 64-bit key per requester (since << 32 | dist << 16 | lane << 8 | movement, all ones for a lane that does not request), a butterfly on
// the key's two halves: every lane of the group evaluates the winner's test on uniform words (conflict[g] and lane[g] are one load each,
// the same address in the whole group), the winning lane takes the result and retires its key.  A round serves one requester of every
// junction of the wavefront; the loop ends when no group of the wavefront has a requester left (one ballot per round), so no lane leaves
// before the last shuffle and a dead group stays for the butterflies.  The group's first lane writes clock, occupied and queued, every
// lane its own grant and since, then the hold.  All lanes of a group sit in one wavefront and the read of clock stands before its write in
// program order, so no lane reads a word another lane of the launch writes.  No LDS, no scratch, no atomics.  Everything it reads is
// device memory, so a replayed hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_reserve_core.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mpcx {

// the minimum of a 64-bit key over the lane group
template <int G>
__device__ __forceinline__ uint64_t group_min_key(uint64_t key) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, m, G), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), m, G);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        key = other < key ? other : key;
    }
    return key;
}

template <int G>
__global__ __launch_bounds__(64) void reserve_kernel(ReserveArgs a) {
    const mpcx_reservation &r = a.rv;
    const int sub = threadIdx.x & (G - 1);
    const int j = blockIdx.x * (64 / G) + (threadIdx.x / G);
    const bool live = j < r.n_junctions;        // (a dead group stays for the butterflies: no lane leaves early)
    const bool mine = live && sub < r.n_per;    // (so does a padding lane of a live group)
    const int q = mine ? j * r.n_per + sub : 0;
    const int32_t k = live ? reserve_mgr(r, j) : -1;
    int32_t t = 0, detect = 0, patience = 0;
    if (k >= 0) {
        t = reserve_clock(r.clock[j]);
        detect = r.mgr_time[2 * (size_t)k];
        patience = r.mgr_time[2 * (size_t)k + 1];
    }
    ReserveMasks mk{0u, 0u, 0u, 0, false};
    int32_t grant = 0, since = -1;
    uint64_t key = MPCX_RESERVE_NO_KEY;
    bool approach = false;
    if (k >= 0 && mine) {
        const ReserveAgent c = reserve_classify(a.s, r, q, detect);
        const ReserveWords w = reserve_request(c, t, sub, r.grant[q], r.since[q]);
        approach = c.kind == MPCX_RESERVE_APPROACH;
        grant = w.grant;
        since = w.since;
        key = w.key;
        mk.occ = w.occ;
    }
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) mk.occ |= (uint32_t)__shfl_xor((int)mk.occ, m, G);
    for (;;) {
        const uint64_t first = group_min_key<G>(key);
        const bool any = first != MPCX_RESERVE_NO_KEY;
        if (__ballot(any) == 0) break;          // wavefront-uniform: every lane has taken part in this round's shuffles
        if (any) {
            mk = reserve_decide(r, first, t, patience, mk);
            if (key == first) {                 // (the lane index is part of the key: one lane of the group)
                if (mk.granted) grant = 1;
                key = MPCX_RESERVE_NO_KEY;
            }
        }
    }
    if (live && sub == 0) {
        if (k >= 0) r.clock[j] = reserve_tick(t);
        r.occupied[j] = (int32_t)mk.occ;
        r.queued[j] = mk.denied;
    }
    if (mine) {
        if (k >= 0) {
            r.grant[q] = grant;
            r.since[q] = since;
        }
        (void)signal_hold(a.s, q, approach, GrantLight{grant});
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no reservations"
bool mpcx_reservation_absent(const mpcx_reservation *s) {
    return !s || (!s->path_exit && !s->conflict && !s->lane && !s->mgr_time && !s->mgr_of && !s->grant && !s->since && !s->clock && !s->occupied &&
                  !s->queued && s->n_per == 0 && s->n_junctions == 0 && s->n_mgr == 0 && s->reserved == 0);
}

// the two structs' own fields and what the reservations need of the run; reads conflict, lane and mgr_time back (never inside a capture).
// exchange: the descriptor's (0 for a stage call); actuated, advised: the run also carries a controller / advice.  Never a GPU fault for a
// bad struct.
int32_t mpcx_reservation_validate(mpcx_ctx *ctx, const mpcx_reservation *s, const mpcx_signals *sg, int32_t P, int32_t exchange, bool actuated,
                                  bool advised) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: null struct");
    if (!sg) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: needs signals (mpcx_signals supplies the stop lines, held and brake)");
    if (sg->plan_cycle || sg->plan_amber || sg->plan_green || sg->plan_of || sg->tick || sg->n_plans != 0)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: the signals also carry a fixed plan (plan_cycle, plan_amber, plan_green, plan_of and tick must be null, n_plans 0): one source of the hold");
    if (actuated) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: the run also carries actuation: one source of the hold");
    if (advised) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: the run also carries advice (there is no plan to look ahead into)");
    const char *missing = !sg->path_stop ? "signals.path_stop" : !sg->path_group ? "signals.path_group" : !sg->held ? "signals.held" :
                          !s->path_exit ? "path_exit" : !s->conflict ? "conflict" : !s->lane ? "lane" : !s->mgr_time ? "mgr_time" :
                          !s->mgr_of ? "mgr_of" : !s->grant ? "grant" : !s->since ? "since" : !s->clock ? "clock" : !s->occupied ? "occupied" :
                          !s->queued ? "queued" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: %s is null (all ten pointers and the signals' path_stop, path_group and held are required)", missing);
    if (sg->n_groups < 1 || sg->n_groups > MPCX_SIGNAL_GROUPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: signals.n_groups = %d outside 1..%d", sg->n_groups, MPCX_SIGNAL_GROUPS_MAX);
    if (sg->n_points < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: signals.n_points = %d, at least one path point", sg->n_points);
    if (!std::isfinite(sg->brake) || !(sg->brake > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: signals.brake = %g must be finite and positive", sg->brake);
    if (sg->reserved != 0 || s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: a reserved word is not 0");
    if (s->n_per < 1 || s->n_per > MPCX_RESERVE_PER_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: n_per = %d outside 1..%d", s->n_per, MPCX_RESERVE_PER_MAX);
    if (s->n_junctions < 0 || (int64_t)s->n_per * (int64_t)s->n_junctions != (int64_t)P)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: n_per * n_junctions = %d * %d is not P = %d", s->n_per, s->n_junctions, P);
    if (s->n_mgr < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: n_mgr = %d, at least one manager", s->n_mgr);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: not supported in the agent-sharded layout (shard by instances)");
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: %d linearisation passes; the stage sits in front of a single window stage", ctx->lin_passes);
    const size_t ng = (size_t)sg->n_groups, nm = (size_t)s->n_mgr;
    std::vector<int32_t> cf(ng), ln(ng), mt(2 * nm);
    if (hipMemcpy(cf.data(), s->conflict, cf.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ln.data(), s->lane, ln.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(mt.data(), s->mgr_time, mt.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "reservation: cannot read the conflict, lane and manager tables back for their check");
    const uint32_t all = (1u << sg->n_groups) - 1u;
    for (size_t g = 0; g < ng; g++) {
        const uint32_t c = (uint32_t)cf[g], l = (uint32_t)ln[g];
        if ((c & ~all) != 0 || (l & ~all) != 0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: movement %d has conflict = 0x%x, lane = 0x%x with bits at or above n_groups = %d", (int)g, c, l, sg->n_groups);
        if ((c >> g) & 1u) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: movement %d conflicts with itself (conflict = 0x%x)", (int)g, c);
        if (!((l >> g) & 1u)) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: lane[%d] = 0x%x lacks its own bit", (int)g, l);
        for (size_t h = 0; h < ng; h++) {
            if (((c >> h) & 1u) != (((uint32_t)cf[h] >> g) & 1u))
                return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: conflict is not symmetric at movements %d and %d", (int)g, (int)h);
            if (((l >> h) & 1u) != (((uint32_t)ln[h] >> g) & 1u))
                return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: lane is not symmetric at movements %d and %d", (int)g, (int)h);
        }
    }
    for (size_t k = 0; k < nm; k++) {
        if (mt[2 * k] < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: manager %d has detect = %d (at least 1 path point)", (int)k, mt[2 * k]);
        if (mt[2 * k + 1] < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "reservation: manager %d has patience = %d", (int)k, mt[2 * k + 1]);
    }
    return MPCX_OK;
}

// the launch alone (the structs have been checked): what the closed loop enqueues behind the conflict search, also inside a capture
int32_t mpcx_reserve_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                             const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const mpcx_signals *signals,
                             const mpcx_reservation *reservation) {
    mpcx::ReserveArgs a;
    memset(&a, 0, sizeof a);
    a.s = mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, *signals};
    a.rv = *reservation;
    const int J = reservation->n_junctions, n = reservation->n_per;
    if (J == 0) return MPCX_OK;
#define MPCX_RSV_LAUNCH(G) hipLaunchKernelGGL(mpcx::reserve_kernel<G>, dim3((J + 64 / G - 1) / (64 / G)), dim3(64), 0, ctx->stream, a)
    if (n <= 1) MPCX_RSV_LAUNCH(1);
    else if (n <= 2) MPCX_RSV_LAUNCH(2);
    else if (n <= 4) MPCX_RSV_LAUNCH(4);
    else if (n <= 8) MPCX_RSV_LAUNCH(8);
    else if (n <= 16) MPCX_RSV_LAUNCH(16);
    else if (n <= 32) MPCX_RSV_LAUNCH(32);
    else MPCX_RSV_LAUNCH(64);
#undef MPCX_RSV_LAUNCH
    return mpcx_check_launch(ctx, "reserve_kernel");
}

extern "C" int32_t mpcx_reserve_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off,
                                           const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                                           const mpcx_signals *signals, const mpcx_reservation *reservation) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "reserve_step_batch: negative size");
    const int32_t rc = mpcx_reservation_validate(ctx, reservation, signals, P, 0, false, false);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !path_len || !traj_idx || !cut_len || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "reserve_step_batch: null buffer (state, path_off, path_len, traj_idx, cut_len) or dl <= 0");
    return mpcx_reserve_enqueue(ctx, P, dl, state, path_off, path_len, traj_idx, cut_len, done, signals, reservation);
}
