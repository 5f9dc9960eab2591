// mpcx_sight.hip -- line of sight in the device-resident closed loop: the struct's checks, the setter that attaches it to the context and the
// stage.  The rule is mpcx_sight_core.h.
// sight_kernel: one launch in front of the conflict search.  A LANE GROUP of SIGHT_G = 16 lanes per agent, four agents per wavefront, as the
// following and the safety stage have it.  Lane j of the group takes the window offsets j, j + 16, ...: a window of at most 16 rows (every
// batch of the stock world) is one pass, the 64 offsets a word holds are four.  Per offset one load of the row's (x, y), the range test,
// and a walk over the occluders of the agent's set: their boxes and half-plane rows are group-uniform addresses of a table of a few KB, so
// every lane of a group issues the same loads and the table lives in the caches.  The word is assembled from the group's 16-bit slice of
// two __ballot words (candidates, seen) per pass; the group's first lane writes the agent's three words.  The trip count of the pass loop is
// group-uniform and only the group's own slice of a ballot is used, so groups that leave early do not disturb the others.  A group whose
// agent is retired writes zeros and leaves at once.  No LDS, no scratch, no atomics; every store is a plain vector store of one lane.
// Why lanes over window offsets and not over (row x occluder): the early exit at the first blocking occluder and the box cull make the
// per-row work short and uneven, and a (row x occluder) mapping would need a second cross-lane reduction per row for a table this small.
#include "mpcx_common.h"
#include "mpcx_sight_core.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mpcx {

constexpr int SIGHT_G = 16;
constexpr int SIGHT_WAVES = 4;

__global__ __launch_bounds__(64 * SIGHT_WAVES) void sight_kernel(SightArgs a) {
    const int sub = threadIdx.x & (SIGHT_G - 1);
    const int slice = SIGHT_G * (int)((threadIdx.x & 63u) / SIGHT_G);       // where the group's lanes sit in a ballot word
    const int q = (int)((blockIdx.x * (unsigned)(64 * SIGHT_WAVES) + threadIdx.x) / SIGHT_G);
    if (q >= a.P) return;
    if (a.done && a.done[q] != 0) {             // (group-uniform)
        if (sub == 0) sight_write(a, q, 0ull, 0ull);
        return;
    }
    int32_t first, last;
    sight_set(a, q, first, last);
    const int n = sight_window(a, q);           // (group-uniform: so is the trip count below)
    unsigned long long seen = 0ull, cand = 0ull;
    for (int base = 0; base < n; base += SIGHT_G) {
        const int j = base + sub;
        const int32_t r = j < n ? sight_candidate(a, q, j) : -1;
        const bool sees = r >= 0 && sight_sees(a, q, r, first, last);
        const unsigned long long bc = __ballot(r >= 0), bs = __ballot(sees);
        cand |= ((bc >> slice) & 0xffffull) << base;
        seen |= ((bs >> slice) & 0xffffull) << base;
    }
    if (sub == 0) sight_write(a, q, seen, cand);
}

}  // namespace mpcx

// all-zero (or no) struct: "no sight stage"
bool mpcx_sight_absent(const mpcx_sight *s) {
    return !s || (!s->sight && !s->n_seen && !s->n_hidden && !s->hp && !s->hp_off && !s->box && !s->set_off && !s->set_of && !s->heard &&
                  s->range == 0.0 && s->n_occ == 0 && s->n_sets == 0 && s->n_rows == 0 && s->n_pool == 0 && s->reserved == 0);
}

// n + 1 offsets on the device: non-decreasing from 0, the last at most `most` (< 0: any).  *end <- the last.
static int32_t sight_check_offsets(mpcx_ctx *ctx, const int32_t *dev, int32_t n, int32_t most, const char *name, int32_t *end) {
    std::vector<int32_t> v((size_t)n + 1);
    if (hipMemcpy(v.data(), dev, v.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "sight: cannot read %s back for its check", name);
    if (v[0] != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: %s[0] = %d is not 0", name, v[0]);
    for (int32_t i = 0; i < n; i++)
        if (v[i + 1] < v[i]) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: %s decreases at %d (%d -> %d)", name, i, v[i], v[i + 1]);
    if (most >= 0 && v[n] > most) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: %s ends at %d, beyond %d", name, v[n], most);
    *end = v[n];
    return MPCX_OK;
}

// the struct's own fields and what the stage needs of the run.  n_pool: the run's pool rows.  Never a GPU fault for a bad struct: the two
// offset tables are read back and checked, set_of is clamped by the rule.  The read-back (two blocking copies) is made once per table:
// ctx->sight_tables remembers the pointers and counts that passed, and mpcx_set_sight forgets them when the struct it is given differs
// from the one it holds -- so a run(1) in a loop checks nothing again, and tables changed in place are checked again after
// mpcx_set_sight(NULL) and a new mpcx_set_sight.  The agent-sharded layout and a descriptor without obs_skip need no test here: the stage
// lives on a scene, and mpcx_scene_validate has refused both before check_stages comes to it.
int32_t mpcx_sight_validate(mpcx_ctx *ctx, const mpcx_sight *s, int32_t P, int32_t n_pool) {
    if (!s) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: null struct");
    const char *missing = !s->sight ? "sight" : !s->n_seen ? "n_seen" : !s->n_hidden ? "n_hidden" : !s->hp_off ? "hp_off" : !s->set_off ? "set_off"
                        : !s->set_of ? "set_of" : nullptr;
    if (missing)
        return mpcx_fail(ctx, MPCX_E_INVALID, "sight: %s is null (sight, n_seen, n_hidden, set_of: n_rows words each; hp_off: n_occ + 1; set_off: n_sets + 1)", missing);
    if (s->n_occ < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: n_occ = %d is negative", s->n_occ);
    if (s->n_sets < 1) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: n_sets = %d, at least one set (an empty one is an open junction)", s->n_sets);
    if (s->n_occ > 0 && (!s->hp || !s->box)) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: hp or box is null with n_occ = %d", s->n_occ);
    if (s->n_rows != P) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: n_rows = %d is not P = %d", s->n_rows, P);
    if (s->n_pool != n_pool) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: n_pool = %d is not the run's %d pool rows", s->n_pool, n_pool);
    if (!(s->range > 0.0)) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: range = %g must be positive (+inf is allowed)", s->range);
    if (s->reserved != 0) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: the reserved word is not 0");
    mpcx_ctx::SightTables &t = ctx->sight_tables;
    if (t.ok && t.set_off == s->set_off && t.hp_off == s->hp_off && t.hp == s->hp && t.n_sets == s->n_sets && t.n_occ == s->n_occ) return MPCX_OK;
    t.ok = false;
    int32_t end = 0;
    int32_t rc = sight_check_offsets(ctx, s->set_off, s->n_sets, s->n_occ, "set_off", &end);
    if (rc != MPCX_OK) return rc;
    rc = sight_check_offsets(ctx, s->hp_off, s->n_occ, -1, "hp_off", &end);
    if (rc != MPCX_OK) return rc;
    if (end > 0 && !s->hp) return mpcx_fail(ctx, MPCX_E_INVALID, "sight: hp is null with %d rows", end);
    t.set_off = s->set_off; t.hp_off = s->hp_off; t.hp = s->hp; t.n_sets = s->n_sets; t.n_occ = s->n_occ; t.ok = true;
    return MPCX_OK;
}

extern "C" int32_t mpcx_set_sight(mpcx_ctx *ctx, const mpcx_sight *s) {
    if (!ctx) return MPCX_E_INVALID;
    mpcx_sight f;
    memset(&f, 0, sizeof f);                                    // (padding too: the cached graph's key takes the struct as it stands)
    const bool have = !mpcx_sight_absent(s);
    if (have) {
        f.sight = s->sight; f.n_seen = s->n_seen; f.n_hidden = s->n_hidden; f.hp = s->hp; f.hp_off = s->hp_off; f.box = s->box;
        f.set_off = s->set_off; f.set_of = s->set_of; f.heard = s->heard; f.range = s->range; f.n_occ = s->n_occ; f.n_sets = s->n_sets;
        f.n_rows = s->n_rows; f.n_pool = s->n_pool; f.reserved = s->reserved;
    }
    if (have != ctx->have_sight || memcmp(&f, &ctx->sight, sizeof f) != 0) ctx->sight_tables.ok = false;    // a new struct: its tables are checked again
    memcpy(&ctx->sight, &f, sizeof f);
    ctx->have_sight = have;
    return MPCX_OK;
}

// the launch alone (the struct has been checked): what the closed loop enqueues, also inside a capture
int32_t mpcx_sight_enqueue(mpcx_ctx *ctx, int32_t P, const double *state, const int32_t *done, int32_t n_obs_pool, const double *obs6,
                           const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip, const int32_t *absent,
                           const mpcx_sight *sight) {
    mpcx::SightArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.n_pool = n_obs_pool;
    a.state = state; a.obs6 = obs6; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip; a.done = done; a.absent = absent;
    a.s = *sight;
    const int per_block = 64 * mpcx::SIGHT_WAVES / mpcx::SIGHT_G;
    hipLaunchKernelGGL(mpcx::sight_kernel, dim3((P + per_block - 1) / per_block), dim3(64 * mpcx::SIGHT_WAVES), 0, ctx->stream, a);
    return mpcx_check_launch(ctx, "sight_kernel");
}

extern "C" int32_t mpcx_sight_step_batch(mpcx_ctx *ctx, int32_t P, const double *state, const int32_t *done, int32_t n_obs_pool,
                                         const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip,
                                         const int32_t *absent, const mpcx_sight *sight) {
    if (!ctx) return MPCX_E_INVALID;
    if (P < 0 || n_obs_pool < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "sight_step_batch: negative size");
    if (!mpcx_sight_absent(sight) && !obs_skip)
        return mpcx_fail(ctx, MPCX_E_INVALID, "sight: no obs_skip (the agents' own pool rows)");
    const int32_t rc = mpcx_sight_validate(ctx, sight, P, n_obs_pool);
    if (rc != MPCX_OK) return rc;
    if (P == 0) return MPCX_OK;
    if (!state || !obs_off || !obs_cnt || (n_obs_pool > 0 && !obs6))
        return mpcx_fail(ctx, MPCX_E_INVALID, "sight_step_batch: null buffer (state, obs6, obs_off, obs_cnt)");
    return mpcx_sight_enqueue(ctx, P, state, done, n_obs_pool, obs6, obs_off, obs_cnt, obs_skip, absent, sight);
}
