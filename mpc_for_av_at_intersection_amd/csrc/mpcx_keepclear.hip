// mpcx_keepclear.hip -- keep clear in the device-resident closed loop: the struct's checks and the stage that holds an agent whose light
// lets it go at its stop line while a conflicting movement is inside the crossing.  The rule is mpcx_keepclear_core.h.
// keepclear_kernel: one launch directly behind signal_kernel / actuated_signal_kernel and in front of the following stage, in both stop
// modes.  The layout is reserve_kernel's: a LANE GROUP of G lanes per junction, G the smallest power of two >= n_per (n_per <= 64), one
// agent per lane, 64 / G junctions per wavefront (a block is one wavefront).  Each lane classifies its agent; one butterfly of __shfl_xor
// within the group ORs the movements inside the crossing, every lane decides for its own agent on that word, and a second butterfly sums
// the agents boxed.  No lane leaves before the last shuffle: a dead group and a padding lane of a live group stay for the butterflies.  The
// group's first lane writes occupied and n_boxed, every lane its own boxed and waited (and lowers its own cut_len).  No lane reads a word
// another lane of the launch writes.  No LDS, no scratch, no atomics, no loop.  Everything it reads is device memory, so a replayed
// hipGraph counts like a plain run.
#include "mpcx_common.h"
#include "mpcx_keepclear_core.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mpcx {

template <int G>
__global__ __launch_bounds__(64) void keepclear_kernel(KeepClearArgs a) {
    const mpcx_keepclear &k = a.kc;
    const int sub = threadIdx.x & (G - 1);
    const int j = blockIdx.x * (64 / G) + (threadIdx.x / G);
    const bool live = j < k.n_junctions;        // (a dead group stays for the butterflies: no lane leaves early)
    const bool mine = live && sub < k.n_per;    // (so does a padding lane of a live group)
    const int q = mine ? j * k.n_per + sub : 0;
    KeepClearAgent c{MPCX_KEEPCLEAR_OUT, 0, 0, 0};
    if (mine) c = keepclear_classify(a.s, k, q);
    uint32_t occ = keepclear_occupies(c);
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) occ |= (uint32_t)__shfl_xor((int)occ, m, G);
    int32_t n = mine ? keepclear_agent(a.s, k, q, c, occ) : 0;
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, G);
    if (live && sub == 0) {
        k.occupied[j] = (int32_t)occ;
        k.n_boxed[j] = n;
    }
}

}  // namespace mpcx

// all-zero (or no) struct: "no keep-clear stage"
bool mpcx_keepclear_absent(const mpcx_keepclear *s) {
    return !s || (!s->path_move && !s->path_exit && !s->conflict && !s->boxed && !s->waited && !s->occupied && !s->n_boxed && s->detect == 0 &&
                  s->n_per == 0 && s->n_junctions == 0 && s->n_moves == 0 && s->n_points == 0 && s->reserved == 0);
}

// the struct's own fields and what the stage needs of the run.  sg: the run's signals (nullptr: none); exchange: the descriptor's (0 for a
// stage call); reserved_run: the run also carries a reservation.  Never a GPU fault for a bad struct.  The conflict table is read back
// (one blocking copy, never inside a capture) ONCE per struct: ctx->keepclear_table remembers the pointer and count that passed, and
// mpcx_set_keepclear forgets them when the struct it is given differs from the one it holds -- so a run(1) in a loop checks nothing again.
int32_t mpcx_keepclear_validate(mpcx_ctx *ctx, const mpcx_keepclear *s, const mpcx_signals *sg, int32_t P, int32_t exchange, bool reserved_run) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: null struct");
    if (!sg) return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: needs signals (mpcx_signals supplies the stop lines, held and brake)");
    if (reserved_run)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: the run also carries a reservation (the manager already keeps the crossing clear: one source of the box rule)");
    const char *missing = !sg->path_stop ? "signals.path_stop" : !sg->held ? "signals.held" : !s->path_move ? "path_move" : !s->path_exit ? "path_exit" :
                          !s->conflict ? "conflict" : !s->boxed ? "boxed" : !s->waited ? "waited" : !s->occupied ? "occupied" :
                          !s->n_boxed ? "n_boxed" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: %s is null (all seven pointers and the signals' path_stop and held are required)", missing);
    if (!std::isfinite(sg->brake) || !(sg->brake > 0.0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: signals.brake = %g must be finite and positive", sg->brake);
    if (s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: the reserved word is not 0");
    if (s->n_per < 1 || s->n_per > MPCX_KEEPCLEAR_PER_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: n_per = %d outside 1..%d", s->n_per, MPCX_KEEPCLEAR_PER_MAX);
    if (s->n_junctions < 0 || (int64_t)s->n_per * (int64_t)s->n_junctions != (int64_t)P)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: n_per * n_junctions = %d * %d is not P = %d", s->n_per, s->n_junctions, P);
    if (s->n_moves < 1 || s->n_moves > MPCX_SIGNAL_GROUPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: n_moves = %d outside 1..%d", s->n_moves, MPCX_SIGNAL_GROUPS_MAX);
    if (s->n_points < 1 || s->n_points != sg->n_points)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: n_points = %d is not the signals' %d path points", s->n_points, sg->n_points);
    if (s->detect < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: detect = %d (at least 1 path point)", s->detect);
    if (exchange == MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: not supported in the agent-sharded layout (shard by instances)");
    if (ctx->lin_passes > 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: %d linearisation passes; the stage sits in front of a single window stage", ctx->lin_passes);
    mpcx_ctx::KeepClearTable &t = ctx->keepclear_table;
    if (t.ok && t.conflict == s->conflict && t.n_moves == s->n_moves) return MPCX_OK;
    t.ok = false;
    const size_t nm = (size_t)s->n_moves;
    std::vector<int32_t> cf(nm);
    if (hipMemcpy(cf.data(), s->conflict, cf.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "keepclear: cannot read the conflict table back for its check");
    const uint32_t all = (1u << s->n_moves) - 1u;
    for (size_t g = 0; g < nm; g++) {
        const uint32_t c = (uint32_t)cf[g];
        if ((c & ~all) != 0)
            return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: movement %d has conflict = 0x%x with bits at or above n_moves = %d", (int)g, c, s->n_moves);
        if ((c >> g) & 1u) return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: movement %d conflicts with itself (conflict = 0x%x)", (int)g, c);
        for (size_t h = 0; h < nm; h++)
            if (((c >> h) & 1u) != (((uint32_t)cf[h] >> g) & 1u))
                return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear: conflict is not symmetric at movements %d and %d", (int)g, (int)h);
    }
    t.conflict = s->conflict; t.n_moves = s->n_moves; t.ok = true;
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_keepclear(mpcx_ctx *ctx, const mpcx_keepclear *s) {
    if (!ctx) return MPCX_E_INVALID;
    mpcx_keepclear f;
    memset(&f, 0, sizeof f);                                    // (padding too: the cached graph's key takes the struct as it stands)
    const bool have = !mpcx_keepclear_absent(s);
    if (have) {
        f.path_move = s->path_move; f.path_exit = s->path_exit; f.conflict = s->conflict; f.boxed = s->boxed; f.waited = s->waited;
        f.occupied = s->occupied; f.n_boxed = s->n_boxed; f.detect = s->detect; f.n_per = s->n_per; f.n_junctions = s->n_junctions;
        f.n_moves = s->n_moves; f.n_points = s->n_points; f.reserved = s->reserved;
    }
    if (have != ctx->have_keepclear || memcmp(&f, &ctx->keepclear, sizeof f) != 0) ctx->keepclear_table.ok = false;    // a new struct: its table is checked again
    memcpy(&ctx->keepclear, &f, sizeof f);
    ctx->have_keepclear = have;
    return MPCX_OK;
}

// the launch alone (the structs have been checked): what the closed loop enqueues behind the hold, also inside a capture
int32_t mpcx_keepclear_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                               const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const mpcx_signals *signals,
                               const mpcx_keepclear *keepclear) {
    mpcx::KeepClearArgs a;
    memset(&a, 0, sizeof a);
    a.s = mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, *signals};
    a.kc = *keepclear;
    const int J = keepclear->n_junctions, n = keepclear->n_per;
    if (J == 0) return MPCX_OK;
#define MPCX_KC_LAUNCH(G) hipLaunchKernelGGL(mpcx::keepclear_kernel<G>, dim3((J + 64 / G - 1) / (64 / G)), dim3(64), 0, ctx->stream, a)
    if (n <= 1) MPCX_KC_LAUNCH(1);
    else if (n <= 2) MPCX_KC_LAUNCH(2);
    else if (n <= 4) MPCX_KC_LAUNCH(4);
    else if (n <= 8) MPCX_KC_LAUNCH(8);
    else if (n <= 16) MPCX_KC_LAUNCH(16);
    else if (n <= 32) MPCX_KC_LAUNCH(32);
    else MPCX_KC_LAUNCH(64);
#undef MPCX_KC_LAUNCH
    return mpcx_check_launch(ctx, "keepclear_kernel");
}

extern "C" int32_t mpcx_keepclear_step_batch(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off,
                                             const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done,
                                             const mpcx_signals *signals, const mpcx_keepclear *keepclear) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear_step_batch: negative size");
    ctx->keepclear_table.ok = false;        // (the struct is the argument's: its table is read back in every stage call)
    const int32_t rc = mpcx_keepclear_validate(ctx, keepclear, mpcx_signals_absent(signals) ? nullptr : signals, P, 0, false);
    ctx->keepclear_table.ok = false;
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !path_off || !path_len || !traj_idx || !cut_len || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "keepclear_step_batch: null buffer (state, path_off, path_len, traj_idx, cut_len) or dl <= 0");
    return mpcx_keepclear_enqueue(ctx, P, dl, state, path_off, path_len, traj_idx, cut_len, done, signals, keepclear);
}
