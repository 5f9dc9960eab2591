// mpcx_interaction_parts.h -- the device side of the conflict search (device-only source, for .hip files): the argument structs, the
// predict_kernel and interaction_kernel templates and the __device__ parts they are made of.  mpcx_interaction.hip instantiates the plain,
// retirement and scene kernels, mpcx_interaction_prec.hip the right-of-way ones.
#pragma once
#include "mpcx_common.h"
#include "mpcx_predict_core.h"

namespace mpcx {

// developer build (make dev): every ego takes the sequential-cumsum path of interaction_kernel, no plan table (tests run both builds)
#ifdef MPCX_INTER_FORCE_EXACT
constexpr bool FORCE_EXACT = true;
#else
constexpr bool FORCE_EXACT = false;
#endif

struct PredArgs {
    mpcx_interaction_params ip;
    int n, n_pool;   // lanes, rows of the pool
    const double *obs6;
    double *pred;    // [n_pool][steps][2][2]
    // closed loop, local pool: the pool row of agent o is packed here from its state and applied inputs (MovingObstacle*.get():
    // x, y, v, yaw, a, steer) instead of by a launch of its own; nullptr: obs6 is read as it is
    const double *pack_state, *pack_applied;
    double *pack_out;
    // closed loop with scripted traffic in the pool (MAPPED instantiation only): lane o < n_ego packs agent o into pool row ego_row[o], lane
    // n_ego + i predicts the row actor_row[i] that traffic_kernel has just written; n = n_ego + n_actors lanes
    const int32_t *ego_row, *actor_row;
    int n_ego;
    // departure (SCENE instantiations only; mpcx_scene::absent, n_pool words): a row with absent[o] != 0 is packed as ever and not predicted --
    // no conflict search reads the prediction of an absent row
    const int32_t *absent;
    // right of way (STAND instantiations only; mpcx_precedence::stand, n_pool rows of four doubles): every predicted row also leaves its
    // STANDING record, the two disc centres of its current pose -- what every frame of the prediction of (x, y, 0, yaw, 0, 0) would hold
    double *stand;
};

// moving_obstacles_prediction.py:21-28, one lane per pool row (predict_row, mpcx_predict_core.h)
template <bool MAPPED, bool SCENE = false, bool STAND = false>
__global__ __launch_bounds__(256) void predict_kernel(PredArgs a) {
    int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= a.n) return;
    double x, y, v, yaw, acc, steer;
    bool pack = a.pack_state != nullptr;
    int src = o;
    if constexpr (MAPPED) {
        pack = o < a.n_ego;
        o = pack ? a.ego_row[o] : a.actor_row[o - a.n_ego];
        if (o < 0 || o >= a.n_pool) return;      // (checked by the host; never written outside the pool)
    }
    if (pack) {
        const double *st = a.pack_state + 4 * (size_t)src;
        x = st[0]; y = st[1]; v = st[2]; yaw = st[3]; acc = a.pack_applied[2 * src + 1]; steer = a.pack_applied[2 * src];
        double *row = a.pack_out + 6 * (size_t)o;
        row[0] = x; row[1] = y; row[2] = v; row[3] = yaw; row[4] = acc; row[5] = steer;
    } else {
        const double *s6 = a.obs6 + 6 * (size_t)o;
        x = s6[0]; y = s6[1]; v = s6[2]; yaw = s6[3]; acc = s6[4]; steer = s6[5];
    }
    if constexpr (SCENE) { if (a.absent[o] != 0) return; }       // (0 <= o < n_pool = the mask's length, checked by the host)
    predict_row<STAND>(a.ip, x, y, v, yaw, acc, steer, STAND ? a.stand + 4 * (size_t)o : nullptr, a.pred + (size_t)o * a.ip.pred_steps * 4);
}

struct InterArgs {
    mpcx_interaction_params ip;
    int P;
    const double *state, *path, *path_cs;
    const int32_t *path_off, *path_len, *prev_cut;
    const double *pred;
    const int32_t *obs_off, *obs_cnt, *obs_skip;
    int32_t *traj_idx, *hit_idx;
    double *hit_xy;
    int32_t *cut_len;
    int max_rem, fcap;    // capacity of this launch: path points ahead of an agent, resampled ego poses (dynamic LDS)
    int32_t *prev_save;   // optional: the previous cut length as read (cut_len may alias prev_cut and is overwritten)
    const int32_t *bin_hint;   // optional (closed loop): file the agent under its work-queue key: bin_cnt[p % COPIES][key]++ -> slot, keyslot[p] = key << 24 | slot
    int32_t *bin_cnt, *keyslot;
    const int32_t *key_prev;   // optional (closed loop, speed-reference mode): what the work-queue key's "moved" test and prev_save take as the previous value of cut_len instead of prev_cut (there prev_cut is the previous PATH length and cut_len the stop index); may alias cut_len
    int32_t *near;        // optional (closed loop): near[3p] = the start index of this agent's nearest-index scan, near[3p+1] / [3p+2] = the largest / smallest of its three nearest indices (absolute), -1 = none
    const int32_t *done;  // retirement (read by the RETIRE instantiation only): done[p] != 0 = agent p has arrived -- no search, no output, not filed in a bin
    const int32_t *absent;    // departure (read by the SCENE instantiation only): absent[r] != 0 = pool row r is not in the scene; n_rows words
    int n_rows;
    // right of way (read by the PREC instantiation only): prec[r] = the precedence word of pool row r, stand[r][4] = its standing record
    const int32_t *prec;
    const double *stand;
};
// line of sight (interaction_sight_kernel only; InterArgs itself stays what it was): sight[p] bit k = agent p sees the row at offset k of its
// window (mpcx_sight.hip)
struct InterSightArgs : InterArgs {
    const unsigned long long *sight;
};

__device__ __forceinline__ double dist2d(double ax, double ay, double bx, double by) {
    const double dx = __dadd_rn(ax, -bx), dy = __dadd_rn(ay, -by);
    return __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
}
// dist2d(a,b) <= md, decided from the squared distance except within 1e-12 (relative) of the threshold, where the
// reference's own expression sqrt(dx*dx + dy*dy) <= md is evaluated: identical decisions, no sqrt on the bulk of the pairs
struct Within {
    double md, md2lo, md2hi;
    __device__ __forceinline__ explicit Within(double md_) : md(md_), md2lo(md_ * md_ * (1.0 - 1e-12)), md2hi(md_ * md_ * (1.0 + 1e-12)) {}
    __device__ __forceinline__ bool operator()(double ax, double ay, double bx, double by) const {
        const double dx = __dadd_rn(ax, -bx), dy = __dadd_rn(ay, -by);
        const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (d2 > md2hi) return false;
        if (d2 < md2lo) return true;
        return __dsqrt_rn(d2) <= md;
    }
};

// ------------------------------------------------------------------------------------------------------------
// collision_avoidance.py:72-104 on prepared disc tables (first_conflict below): run_boxes, first_row, earliest_pose.
//
// Work distribution.  The reference's row order is frame-major, so the answer lies in the FIRST run of ego frames that has any hit:
// runs are visited in order and the search stops after the first run with a hit.  Per run, every lane tests the obstacle disc
// positions it holds in registers (8 per lane = 512 per chunk, one global load each) against the run's inflated box into a bit mask and
// works its own set bits off, all lanes on the same ego frame, leaving at the first frame with a hit anywhere in the wavefront
// (round 1: one position per lane through all runs with nested divergent loops; rounds 2-3: survivors compacted into an LDS queue).
constexpr int NSEG = 8;
constexpr int SPARE_ROWS = 32;      // rows of four doubles the launch keeps free behind s_ego [fcap][4]: the first NSEG of them are s_box
__device__ __forceinline__ double grp8_min(double v) {
    v = fmin(v, dpp_mov<0xB1>(v, v)); v = fmin(v, dpp_mov<0x4E>(v, v)); v = fmin(v, dpp_mov<0x141>(v, v));
    return v;
}
__device__ __forceinline__ double grp8_max(double v) {
    v = fmax(v, dpp_mov<0xB1>(v, v)); v = fmax(v, dpp_mov<0x4E>(v, v)); v = fmax(v, dpp_mov<0x141>(v, v));
    return v;
}
// j / d and j % d for 0 <= j < 2^20, 1 <= d <= MPCX_PRED_STEPS_MAX through the single-precision reciprocal (+ one correction either way):
// the integer division the compiler emits costs ~25 instructions, and the candidate decode below runs it sixteen times per lane in a
// kernel that is bound by instruction issue
__device__ __forceinline__ void divmod_small(int j, int d, float inv_d, int &quo, int &rem) {
    int q = (int)(((float)j + 0.5f) * inv_d);
    int r = j - q * d;
    if (r < 0) { q -= 1; r += d; }
    if (r >= d) { q += 1; r -= d; }
    quo = q; rem = r;
}

// Boxes of NSEG runs of ego frames (F frames padded, SL per run), inflated by slack > md so that no pair within md is ever skipped.
// Lane (run = lane / 8, j = lane % 8) folds frames run*SL + j, + 8, ...; an 8-lane butterfly finishes the run.
__device__ __forceinline__ void run_boxes(const double (*s_ego)[4], int na, int F, int SL, double slack, double (*s_box)[4], int lane) {
    const int sg = lane >> 3, j = lane & 7;
    const int fend = (sg + 1) * SL < F ? (sg + 1) * SL : F;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int f = sg * SL + j; f < fend; f += 8) {
        const int fe = f < na ? f : na - 1;
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const double ex = s_ego[fe][2 * d], ey = s_ego[fe][2 * d + 1];
            x0 = fmin(x0, ex); x1 = fmax(x1, ex); y0 = fmin(y0, ey); y1 = fmax(y1, ey);
        }
    }
    x0 = grp8_min(x0); x1 = grp8_max(x1); y0 = grp8_min(y0); y1 = grp8_max(y1);
    if (j == 0) { s_box[sg][0] = x0 - slack; s_box[sg][1] = x1 + slack; s_box[sg][2] = y0 - slack; s_box[sg][3] = y1 + slack; }
}

// departure (mpcx_scene): the obstacle list of an agent as the window offsets (< 64, six bits each) of the PRESENT rows of its window in rank
// order, at most MPCX_MAX_OBS of them, packed into two wave-uniform words (ten + six entries): scalar registers, no LDS, and the
// candidate -> pool row lookup in first_row's load loop is a shift and a mask with no memory wait in front of the loads it feeds.
struct RowList {
    unsigned long long lo, hi;
    static constexpr int PER = 10, BITS = 6;
    static_assert(MPCX_MAX_OBS <= PER + 64 / BITS, "two words do not hold the list");
    // m: bit k set = row (window offset) k is present; wave-uniform, at most MPCX_MAX_OBS bits set
    static __device__ __forceinline__ RowList of(unsigned long long m) {
        RowList l = {0, 0};
        for (int r = 0; m; r++, m &= m - 1) {
            const unsigned long long k = (unsigned long long)(__ffsll((long long)m) - 1);
            if (r < PER) l.lo |= k << (BITS * r); else l.hi |= k << (BITS * (r - PER));
        }
        return l;
    }
    __device__ __forceinline__ int operator[](int o) const {
        const bool first = o < PER;
        return (int)(((first ? lo : hi) >> (BITS * (first ? o : o - PER))) & 63ull);
    }
};
// collision_avoidance.py:72-87: the first row of the pair table within md, as the minimum of a key in the reference's row order.
// Returns whether there is one; (hox, hoy): the obstacle disc position of that row.
// SCENE: candidate rank o is the o-th PRESENT row of the window, rows[o] its offset in the window (present_rows below); nobs counts those.
// PREC (with SCENE): bit o of `yields` set = the row of rank o yields to this agent, which sees it STANDING: every frame of its prediction is
// its standing record stand[pool][4] -- the candidate's address is selected between the two tables, everything after the load is the same.
template <bool SCENE = false, bool PREC = false>
__device__ __forceinline__ bool first_row(const mpcx_interaction_params &ip, const Within &within, const double (*s_ego)[4], int na, int F, int SL,
                                          const double (*s_box)[4], const double *pred, int ooff, int nobs, int oskip, int lane,
                                          double &hox, double &hoy, const RowList rows = {0, 0}, const double *stand = nullptr,
                                          unsigned yields = 0u) {
    const int steps = ip.pred_steps, w = ip.frame_window;
    const float inv_steps = 1.0f / (float)steps;
    const long long NOKEY = 0x7fffffffffffffffLL;
    long long lbest = NOKEY;                               // this lane's own smallest key and the obstacle disc position it belongs to
    double lpx = 0.0, lpy = 0.0;
    int sg_limit = NSEG;                                   // runs >= sg_limit cannot hold the first row any more
    const int ncand_all = nobs * steps * 2;
    for (int cb = 0; cb < ncand_all; cb += 8 * WAVE) {
        double ox[8], oy[8];
        // all eight loads of the lane in flight at once, from addresses that are valid for every lane (clamped); out-of-range
        // candidates become +inf afterwards (a load under a lane predicate is its own exec-masked block with a full wait)
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int cidx = cb + u * WAVE + lane;
            const int cc = cidx < ncand_all ? cidx : ncand_all - 1;
            const int co = cc & 1;
            int g, o;                                                              // o: local obstacle rank
            divmod_small(cc >> 1, steps, inv_steps, o, g);
            int pool;
            if constexpr (SCENE) pool = ooff + rows[o];                                    // the list leaves out self and the absent rows
            else {
                pool = ooff + o;
                if (oskip >= 0 && pool >= oskip) pool += 1;                                // skip self
            }
            const double *qq = pred + ((size_t)pool * steps + g) * 4 + 2 * co;
            if constexpr (PREC) {
                const double *qs = stand + (size_t)pool * 4 + 2 * co;
                qq = ((yields >> o) & 1u) ? qs : qq;                                       // a select, not a branch: one load either way
            }
            ox[u] = qq[0]; oy[u] = qq[1];
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (cb + u * WAVE + lane >= ncand_all) { ox[u] = INFINITY; oy[u] = INFINITY; }       // fails every box test
        for (int sg = 0; sg < sg_limit; sg++) {             // wave-uniform
            const double b0 = s_box[sg][0], b1 = s_box[sg][1], b2 = s_box[sg][2], b3 = s_box[sg][3];
            // Round 4: no queue.  Which of the lane's eight positions lie in the run's box is a bit mask, and every lane works its OWN set bits
            // off, one per pass (consecutive candidates -- the frames and discs of one obstacle -- sit on consecutive lanes, so the positions
            // inside a box are spread over the lanes: one or two passes).  The compaction into an LDS queue cost a ballot, two pop counts
            // and a store per position and run, two barriers per run, and a RELOAD of every queued position (one more memory round trip per
            // run visited, in a kernel whose time is a chain of such round trips).
            unsigned mask = 0;
#pragma unroll
            for (int u = 0; u < 8; u++)
                mask |= (unsigned)((ox[u] >= b0) & (ox[u] <= b1) & (oy[u] >= b2) & (oy[u] <= b3)) << u;
            if (!__ballot(mask != 0u)) continue;
            const int f0 = sg * SL;
            int f1 = (sg + 1) * SL < F ? (sg + 1) * SL : F;
            bool found = false;
            while (__ballot(mask != 0u)) {                  // wave-uniform: as many passes as the busiest lane has positions in the box
                const bool on = mask != 0u;
                const int u = on ? __ffs((int)mask) - 1 : 0;
                mask &= mask - 1;
                double px = ox[0], py = oy[0];
#pragma unroll
                for (int q = 1; q < 8; q++) { px = (u == q) ? ox[q] : px; py = (u == q) ? oy[q] : py; }
                const int cidx = cb + u * WAVE + lane;
                const int co = cidx & 1;
                int g, o;
                divmod_small(cidx >> 1, steps, inv_steps, o, g);
                // frame-major, all lanes on the same frame: the key is ordered by the frame first, so once ANY lane has a hit at frame f no
                // later frame can hold the first row -- this pass ends with frame f, and later passes need not look beyond it
                for (int f = f0; f < f1; f++) {             // wave-uniform bounds
                    const int ff = f < steps ? f : steps - 1;
                    const int fe = f < na ? f : na - 1;
                    bool hit = false;
                    if (on && abs(g - ff) <= w) {            // else: no offset d in [-w, w] maps padded frame ff onto obstacle frame g
#pragma unroll
                        for (int ca = 0; ca < 2; ca++) {
                            if (within(s_ego[fe][2 * ca], s_ego[fe][2 * ca + 1], px, py)) {
                                // key = reference row order (frame, agent disc, obstacle, offset, obstacle disc); offsets ascend =>
                                // obstacle frames descend; the first offset reaching g is the one that counts
                                const long long key = ((((long long)f * 2 + ca) * MPCX_MAX_OBS + o) * MPCX_PRED_STEPS_MAX + (steps - 1 - g)) * 2 + co;
                                if (key < lbest) { lbest = key; lpx = px; lpy = py; }
                                hit = true;
                            }
                        }
                    }
                    if (__ballot(hit)) { found = true; f1 = f + 1; break; }
                }
            }
            if (__ballot(found)) {                         // rows of later runs come later in the reference's order
                sg_limit = sg + 1;                         // later chunks: only runs up to this one can still win
                break;
            }
        }
    }
    const long long best = wave_min_i(lbest);
    if (best == NOKEY) return false;
    // the obstacle disc of the first row: the lane that found the key still holds its position (a key belongs to one candidate, a
    // candidate to one lane) -- no decode, no load
    const int owner = (int)__ffsll((long long)__ballot(lbest == best)) - 1;
    hox = rdlane(lpx, owner); hoy = rdlane(lpy, owner);
    return true;
}

// collision_avoidance.py:88-104: earliest pose of the detailed path (front-disc block, then rear-disc block) within md of (ox, oy).
// The answer is the smallest index of the front-disc block if that block has a hit at all, else the smallest of the
// rear-disc block: each block is walked in index order, 64 poses at a time, and left at the first batch with a hit.
__device__ __forceinline__ int earliest_pose(const mpcx_interaction_params &ip, const Within &within, double ox, double oy, const double *rem,
                                             const double *rcs, const double *pdisc, int n, int lane) {
    int first = 0x7fffffff;
    constexpr int PD = 4;      // batches of 64 poses in flight: the scan leaves at its first hit, and one batch per memory round trip made it a chain of 2-5
    for (int d = 0; d < 2 && first == 0x7fffffff; d++) {
        const double cx = ip.circle_centers[2 * d], cy = ip.circle_centers[2 * d + 1];
        for (int i0 = 0; i0 < n && first == 0x7fffffff; i0 += PD * WAVE) {
            double px[PD], py[PD], pc[PD], ps[PD];
#pragma unroll
            for (int k = 0; k < PD; k++) {
                const int i = i0 + k * WAVE + lane;
                const int ic = i < n ? i : n - 1;             // clamped address, masked below
                if (pdisc) { px[k] = pdisc[4 * (size_t)ic + 2 * d]; py[k] = pdisc[4 * (size_t)ic + 2 * d + 1]; pc[k] = 0.0; ps[k] = 0.0; }
                else { px[k] = rem[3 * ic]; py[k] = rem[3 * ic + 1]; pc[k] = rcs[2 * ic]; ps[k] = rcs[2 * ic + 1]; }
            }
#pragma unroll
            for (int k = 0; k < PD; k++) {
                const int i = i0 + k * WAVE + lane;
                // (with the host's table the disc centre is read, not rebuilt: px, py hold it)
                double ex, ey;
                disc_centre(px[k], py[k], pc[k], ps[k], cx, cy, ex, ey);
                ex = pdisc ? px[k] : ex; ey = pdisc ? py[k] : ey;
                const bool hit = i < n && within(ox, oy, ex, ey);
                const unsigned long long m = __ballot(hit);
                if (m && first == 0x7fffffff) first = d * n + i0 + k * WAVE + (int)__ffsll((long long)m) - 1;      // wave-uniform
            }
        }
    }
    return (first == 0x7fffffff) ? 0 : first % n;      // argmax of an all-False mask is 0
}

// s_ego: ego disc centres of the `na` predicted poses; pred: obstacle disc centres [pool][steps][2][2]; (rem, rcs, n): the detailed path and
// cos/sin of its yaw.  Returns the index of the earliest conflicting pose on the detailed path (and its x,y) or -1 (None).
template <bool SCENE = false, bool PREC = false>
__device__ int first_conflict(const mpcx_interaction_params &ip, double (*s_ego)[4], int na, const double *pred,
                              int ooff, int nobs, int oskip, const double *rem, const double *rcs, int n,
                              double (*s_box)[4], int lane, double &hx, double &hy,
                              bool boxes_ready = false,          // s_box already holds the runs' boxes (mpcx_interaction_params.plan_box)
                              const double *pdisc = nullptr,     // disc centres of the poses of `rem` (mpcx_interaction_params.path_disc + 4 * row of rem[0]) or nullptr
                              const RowList rows = {0, 0},       // SCENE: the window offsets of the nobs present rows
                              const double *stand = nullptr, unsigned yields = 0u     // PREC: the standing records and who yields, by rank
                              ) {
    const Within within(2.0 * ip.radius);
    const double slack = within.md * (1.0 + 1e-9) + 1e-9;      // conservative: never culls a pair within md
    const int F = na > ip.pred_steps ? na : ip.pred_steps;
    const int SL = (F + NSEG - 1) / NSEG;                 // frames per run
    if (!boxes_ready) run_boxes(s_ego, na, F, SL, slack, s_box, lane);
    __syncthreads();
    double ox, oy;
    if (!first_row<SCENE, PREC>(ip, within, s_ego, na, F, SL, s_box, pred, ooff, nobs, oskip, lane, ox, oy, rows, stand, yields)) return -1;
    const int first = earliest_pose(ip, within, ox, oy, rem, rcs, pdisc, n, lane);
    hx = rem[3 * first]; hy = rem[3 * first + 1];
    return first;
}

// lane 0: the agent's outputs and, next to the store of cut_len, its place in the QP work queue of this step (closed loop: an agent that
// is not filed is never solved)
__device__ __forceinline__ void finish(const InterArgs &a, int p, int lane, int kprev, int hit, double hx, double hy, int cl) {
    if (lane != 0) return;
    a.hit_idx[p] = hit; a.cut_len[p] = cl;
    if (a.bin_cnt) {
        const int k = order_key_of(a.bin_hint ? a.bin_hint[p] : 0, cl != kprev);
        a.keyslot[p] = (k << 24) | atomicAdd(&a.bin_cnt[(p % MPCX_ORDER_COPIES) * MPCX_ORDER_BINS + k], 1);
    }
    a.hit_xy[2 * p] = hx; a.hit_xy[2 * p + 1] = hy;
}
// no conflict (-1), beyond the launch's capacity (-2), the reference's 'something wrong' (-3): the path stays whole
__device__ __forceinline__ void leave(const InterArgs &a, int p, int lane, int kprev, int len, int code) { finish(a, p, lane, kprev, code, 0, 0, len); }

// mpc_intersection.py:103-105: advance traj_agent_idx unless the previous tmp_trajectory collapsed onto it.  Returns the new index, or the
// exit code: -2 beyond the launch's capacity, -3 where the reference raises (trajectories.py:126).  Without the arc-length table it also
// leaves the step lengths of path[t_old ..] in s_cum.
constexpr int DEPTH = 4;
__device__ __forceinline__ int locate(const InterArgs &a, int p, int lane, const double *path, int len, int t_old, double x, double y,
                                      int pcut, int nobs, bool tab, double *s_cum) {
    const int MAXREM = a.max_rem, n_old = len - t_old;
    if (a.near && lane == 0) { a.near[3 * p] = t_old; a.near[3 * p + 1] = -1; a.near[3 * p + 2] = -1; }       // until the scan below has an answer
    // The first batches of the distance pass are requested BEFORE it is known whether the ego advances at all (their addresses need only the
    // path and the old index): they travel together with the six values of the test below instead of one memory round trip later.  The
    // test itself loads all six values and compares them without short-circuit branches -- (a != b) || (c != d) || ... is a chain of up
    // to three dependent round trips for exactly the egos that stand still.
    double bx[DEPTH], by[DEPTH];
#pragma unroll
    for (int k = 0; k < DEPTH; k++) {
        const int i = k * WAVE + lane;
        const double *q = path + 3 * (size_t)(t_old + ((i < n_old && n_old <= MAXREM) ? i : 0));       // clamped address, selected afterwards
        const double vx = q[0], vy = q[1];
        bx[k] = i < n_old ? vx : 0.0; by[k] = i < n_old ? vy : 0.0;
    }
    const int last = pcut > 0 ? pcut - 1 : t_old;
    const double ax = path[3 * t_old], ay = path[3 * t_old + 1], ath = path[3 * t_old + 2];
    const double lx = path[3 * last], ly = path[3 * last + 1], lth = path[3 * last + 2];
    const bool advance = (pcut <= 0) | (ax != lx) | (ay != ly) | (ath != lth);
    if (n_old > MAXREM || nobs > MPCX_MAX_OBS) return -2;
    // ONE pass over the remaining path: distances to the ego (per-lane three smallest, ties by lower index: Top3) for
    // trajectories.py:100-126, and the step lengths |p_i - p_{i-1}| for resample_curve (trajectories.py:72-75).
    // Each point is loaded once (the predecessor comes from the neighbour lane) and the next 64 points are in flight while
    // the current ones are worked on.
    // With the caller's arc-length table (mpcx_interaction_params.path_cum) the step lengths are not needed here at all -- no
    // square root, no neighbour shuffles, nothing stored -- and an agent that does not advance skips the pass.
    Top3 top;
    if (!tab || advance) {
        // the points arrive in batches of DEPTH x 64: the loads of the next batch are all in flight while this one is worked on (one
        // batch deep the pass waited for an L2 round trip per 64 points: it is bound by its loads, not by its arithmetic)
        double lastx = 0.0, lasty = 0.0;
        for (int i0 = 0; i0 < n_old; i0 += DEPTH * WAVE) {
            double nbx[DEPTH], nby[DEPTH];
#pragma unroll
            for (int k = 0; k < DEPTH; k++) {
                const int i = i0 + (DEPTH + k) * WAVE + lane;
                const double *q = path + 3 * (size_t)(t_old + (i < n_old ? i : 0));
                const double vx = q[0], vy = q[1];
                nbx[k] = i < n_old ? vx : 0.0; nby[k] = i < n_old ? vy : 0.0;
            }
#pragma unroll
            for (int k = 0; k < DEPTH; k++) {
                const int i = i0 + k * WAVE + lane;
                const double px = bx[k], py = by[k];
                if (!tab) {
                    double qx = __shfl_up(px, 1, WAVE), qy = __shfl_up(py, 1, WAVE);
                    if (lane == 0) { qx = lastx; qy = lasty; }
                    lastx = rdlane(px, WAVE - 1); lasty = rdlane(py, WAVE - 1);
                    if (i < n_old) s_cum[i] = (i == 0) ? 0.0 : dist2d(px, py, qx, qy);
                }
                if (i < n_old && advance) top.offer(px, py, x, y, i);
            }
#pragma unroll
            for (int k = 0; k < DEPTH; k++) { bx[k] = nbx[k]; by[k] = nby[k]; }
        }
    }
    int tidx = t_old;
    if (advance && n_old == 2) tidx = t_old + 1;
    else if (advance && n_old > 2) {
        int bi[3];
        top.pop3(bi);
        tidx = three_nearest(bi, t_old);
        if (a.near && lane == 0 && tidx >= 0) { a.near[3 * p + 1] = t_old + max(bi[0], max(bi[1], bi[2])); a.near[3 * p + 2] = t_old + min(bi[0], min(bi[1], bi[2])); }
    }
    return tidx < 0 ? -3 : tidx;
}

struct Ego {                       // what the resampling parts share about one ego (wave-uniform but for the lane)
    const mpcx_interaction_params &ip;
    int lane, MAXF;
    double *s_cum;                 // LDS: step / cumulative lengths, s_cum[shift + i] belongs to point i of the trajectory
    unsigned short *s_keep;        // LDS: indices of the kept poses
    const double *cumtab;          // the caller's arc-length table from the path's first point on, or nullptr
    const double *rem;             // trajectory = trajectory_full[traj_agent_idx:], n points
    int tidx, shift, n;
    double v;
    bool accel_phase;              // the predicted speed v + a (i + 1) starts below max_speed
    double dl_const, inv_const;    // dl once it has saturated: dt * max_speed, and its reciprocal
    double cum0;                   // the table's value at the trajectory's first point
    double marg;                   // how far the fast running sum can be from np.cumsum's
};

// ---- mpc_intersection.py:110-116 + trajectories.py:72-86: ego prediction = resample_curve(trajectory, dl_k).
// np.cumsum adds strictly left to right.  Replaying that on one lane cost a third of this kernel, so the cumulative
// lengths first come from a PARALLEL scan (all terms >= 0: it differs from the sequential sum by <= 2.4e-11 for 1024
// terms summing to <= 200 m) and the bucket floor(c_i / dl_i) of every point is accepted only when c_i / dl_i is farther
// from an integer than that error can move it (margin 1e-10 / dl_i).  If a single point of this ego is too close to call,
// the ego is redone with the sequential sum -- same outputs as before in every case, about 1e-6 of the egos take that path.
__device__ __forceinline__ void prefix_fast(const Ego &e) {
    double carry = 0.0;
    for (int i0 = 0; i0 < e.n; i0 += WAVE) {
        const int i = i0 + e.lane;
        double t = (i >= 1 && i < e.n) ? e.s_cum[e.shift + i] : 0.0;     // the first point of the new trajectory has no predecessor
        t += dpp_mov<0x111>(0.0, t);
        t += dpp_mov<0x112>(0.0, t);
        t += dpp_mov<0x114>(0.0, t);
        t += dpp_mov<0x118>(0.0, t);
        t += dpp_mov<0x142, 0xA>(0.0, t);       // row_bcast:15 -> rows 1, 3
        t += dpp_mov<0x143, 0xC>(0.0, t);       // row_bcast:31 -> rows 2, 3
        t += carry;
        carry = rdlane(t, WAVE - 1);
        if (i < e.n) e.s_cum[e.shift + i] = t;
    }
}
// running sums from the table, four batches of loads in flight (one by one the pass waited a memory round trip per 64 points)
__device__ __forceinline__ void sums_from_table(const Ego &e) {
    for (int i0 = 0; i0 < e.n; i0 += 4 * WAVE) {
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const int i = i0 + k * WAVE + e.lane; t[k] = e.cumtab[e.tidx + (i < e.n ? i : 0)]; }
#pragma unroll
        for (int k = 0; k < 4; k++) { const int i = i0 + k * WAVE + e.lane; if (i < e.n) e.s_cum[e.shift + i] = t[k] - e.cum0; }
    }
}
__device__ __forceinline__ void prefix_exact(const Ego &e) {
    const int n = e.n, shift = e.shift;
    double *s_cum = e.s_cum;
    for (int i = e.lane; i < n; i += WAVE) {        // the step lengths again (prefix_fast overwrote them)
        const double *q = e.rem + 3 * (size_t)i;
        s_cum[shift + i] = (i == 0) ? 0.0 : dist2d(q[0], q[1], q[-3], q[-2]);
    }
    __syncthreads();
    if (e.lane == 0) {                      // np.cumsum: strictly sequential adds (one lane; loads batched 16 at a time)
        double c = 0.0;
        int i = 1;
        for (; i + 16 <= n; i += 16) {
            double t[16];
#pragma unroll
            for (int q = 0; q < 16; q++) t[q] = s_cum[shift + i + q];
#pragma unroll
            for (int q = 0; q < 16; q++) { c = __dadd_rn(c, t[q]); t[q] = c; }
#pragma unroll
            for (int q = 0; q < 16; q++) s_cum[shift + i + q] = t[q];
        }
        for (; i < n; i++) { c = __dadd_rn(c, s_cum[shift + i]); s_cum[shift + i] = c; }
    }
    __syncthreads();
}
// the fast sums' bucket floor(r), r = c * inv, is not safe to take for np.cumsum's floor(c / dl)
__device__ __forceinline__ bool risky(const Ego &e, double c, double r, double dl, double inv) {
    return c != 0.0 && (!(dl > 0.0) || !(r < 4e15) || !(fabs(r - rint(r)) > e.marg * inv + 2e-15 * fabs(r)));      // c == 0 is exact in every summation order
}
// does the predicted speed of point i stay below max_speed (dl_i is not the constant yet)?  Monotone in i for max_accel >= 0.
__device__ __forceinline__ bool below_max_speed(const Ego &e, int i) {
    return e.accel_phase && (!(e.ip.max_accel >= 0.0) || __dadd_rn(__dmul_rn(e.ip.max_accel, (double)(i + 1)), e.v) < e.ip.max_speed);
}

// Point by point over the sums in s_cum: bucket of every point, keep the points where the bucket advances (+ first and last); returns the
// number kept.  Two instantiations: the fast pass carries no division and no 64-bit integers.
// check = true: the fast pass -- running sums from the table (or the parallel scan), quotient by reciprocal (<= 2 ulp from the
// division), bucket accepted only outside the margin; check = false: np.cumsum's own sums (prefix_exact) and the division
template <bool check>
__device__ __forceinline__ int resample_by_scan(const Ego &e, bool &unsure) {
    const mpcx_interaction_params &ip = e.ip;
    const int lane = e.lane, n = e.n;
    int base = 0;
    long long q_carry = 0;                // bucket of the last element of the previous 64-block
    double qd_carry = 0.0;                // (fast pass: the buckets as doubles -- floor() of a quotient below 2^52 is an exact integer)
    unsure = false;
    for (int i0 = 0; i0 < n; i0 += WAVE) {
        const int i = i0 + lane;
        long long q = 0;
        double qd = 0.0;
        if (i < n) {
            double dl = e.dl_const, inv = e.inv_const;
            // the predicted speed v + a (i + 1) is monotone in i: once the FIRST point of a 64-point block has reached max_speed every
            // later one has, and dl is the constant (a car needs four points for that: only the first block takes this branch)
            if (below_max_speed(e, i0)) {
                const double r = __dadd_rn(__dmul_rn(ip.max_accel, (double)(i + 1)), e.v);   // cumsum of equal terms (exact for 2.0) + v
                dl = __dmul_rn(ip.dt, fmin(r, ip.max_speed));
                if (check) inv = frcp(dl);
            }
            const double c = e.s_cum[e.shift + i];
            if constexpr (check) {
                const double r = c * inv;
                qd = floor(r);
                if (risky(e, c, r, dl, inv)) unsure = true;
            } else
                q = (long long)floor(__ddiv_rn(c, dl));
        }
        bool adv;
        if constexpr (check) {
            const double qprev = lane_prev(qd, qd_carry);       // wave_shr:1, lane 0 takes the previous block's last bucket
            qd_carry = rdlane(qd, WAVE - 1);
            adv = qd - qprev >= 1.0;
        } else {
            long long qprev = __shfl_up(q, 1, WAVE);
            if (lane == 0) qprev = q_carry;
            q_carry = __shfl(q, WAVE - 1, WAVE);
            adv = q - qprev >= 1;
        }
        const bool keep = (i < n) && ((i == 0) || (i == n - 1) || adv);
        const unsigned long long m = __ballot(keep);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < e.MAXF) e.s_keep[pos] = i;
        base += __popcll(m);
    }
    return base;
}

// Round 4: the kept poses by SEARCH instead of a scan.  Beyond the first 64 points dl is a constant (the predicted speed has saturated), so
// the buckets floor(c_i / dl) never decrease along the path and the kept points -- those whose bucket exceeds their predecessor's -- are
// the FIRST point of every bucket value that occurs: one binary search in the arc-length table per bucket boundary (~36 of them, one per
// lane) instead of a pass over all ~700 points (which was a third of this kernel's instructions), and the table no longer goes through
// LDS.  The margin test that guards the fast sums is only needed where it can fail: at the two points around every boundary and at
// the last point (a quotient close to an integer m elsewhere would put a boundary point at least as close to m).  First 64 points: as
// before, point by point (dl varies there while the ego accelerates).  Same kept set as the scan, bit for bit (tests + the
// MPCX_INTER_FORCE_EXACT build, which still takes the sequential path).  Needs the table, n > 64 and the constant dl from point 64 on.
__device__ __forceinline__ int resample_by_search(const Ego &e, bool &unsure) {
    const int lane = e.lane, n = e.n, MAXF = e.MAXF;
    const double dl_const = e.dl_const, inv_const = e.inv_const, cum0 = e.cum0;
    unsigned short *s_keep = e.s_keep;
    const double *ct = e.cumtab + e.tidx;
    unsure = false;
    // ---- points 0..63 (n > 64: none of them is the last point)
    double dl = dl_const, inv = inv_const;
    if (below_max_speed(e, 0)) {
        const double r = __dadd_rn(__dmul_rn(e.ip.max_accel, (double)(lane + 1)), e.v);
        dl = __dmul_rn(e.ip.dt, fmin(r, e.ip.max_speed));
        inv = frcp(dl);
    }
    const double c0 = ct[lane] - cum0;
    const double r0 = c0 * inv;
    const double qd = floor(r0);
    if (risky(e, c0, r0, dl, inv)) unsure = true;
    const double qprev = lane_prev(qd, 0.0);
    const bool keep0 = (lane == 0) || (qd - qprev >= 1.0);
    const unsigned long long m0 = __ballot(keep0);
    {
        const int pos = __popcll(m0 & ((1ull << lane) - 1ull));
        if (keep0 && pos < MAXF) s_keep[pos] = lane;
    }
    int base = __popcll(m0);
    const double Q63 = rdlane(qd, WAVE - 1);
    // ---- point 64 (the first with the constant dl) and the last point
    const double c64 = ct[WAVE] - cum0, cl = ct[n - 1] - cum0;
    const double r64 = c64 * inv_const, rl = cl * inv_const;
    const double Q64 = floor(r64), Ql = floor(rl);
    if (risky(e, c64, r64, dl_const, inv_const) || risky(e, cl, rl, dl_const, inv_const)) unsure = true;
    if (__ballot(unsure)) return base;                    // (wave-uniform) the caller redoes the ego with the sequential sums
    if ((Q64 - Q63 >= 1.0) || n - 1 == WAVE) {
        if (lane == 0 && base < MAXF) s_keep[base] = WAVE;
        base++;
    }
    // ---- one target bucket value per lane: idx(b) = first i in [65, n) with floor(c_i / dl) >= b, b = Q64 + 1 .. Ql
    const int ntar = (int)(Ql - Q64);                     // 0 <= ntar: the buckets do not decrease; < 4e15 checked above
    int last_idx = WAVE;                                  // the largest index handled so far
    if (ntar > 0) {
        int span = n - 1 - (WAVE + 1), iters = 0;         // search range [65, n - 1]: r_{n-1} >= Ql >= b, so the answer exists
        while (span > 0) { iters++; span >>= 1; }
        // planner paths are sampled at (nearly) equal arc-length steps, so the boundary is where a straight line through c_64 and
        // c_{n-1} puts it: ONE probe of the two points around the guess -- they are the two points the margin test needs anyway --
        // instead of a chain of ~10 dependent loads; the binary search remains for a path on which the guess misses
        const double hstep = (cl - c64) / (double)(n - 1 - WAVE);
        const double inv_h = hstep > 0.0 ? 1.0 / hstep : 0.0;
        for (int t0 = 0; t0 < ntar; t0 += WAVE) {
            const int t = t0 + lane;
            const bool valid = t < ntar;
            const double b = valid ? Q64 + 1.0 + (double)t : Ql;
            double gd = ceil((b * dl_const - c64) * inv_h) + (double)WAVE;
            gd = fmin(fmax(gd, (double)(WAVE + 1)), (double)(n - 1));
            int idx = (int)gd;
            double cj = ct[idx] - cum0, ci = ct[idx - 1] - cum0;
            const bool miss = valid && !((ci * inv_const < b) && (cj * inv_const >= b));
            if (__ballot(miss)) {                         // wave-uniform
                int lo = miss ? WAVE + 1 : idx, hi = miss ? n - 1 : idx;
                for (int it = 0; it < iters; it++) {      // uniform trip count; a lane that has converged repeats its last probe
                    const int mid = lo < hi ? (lo + hi) >> 1 : lo;
                    const double cm = ct[mid] - cum0;
                    const bool ge = cm * inv_const >= b;
                    if (lo < hi) { if (ge) hi = mid; else lo = mid + 1; }
                }
                idx = lo;
                cj = ct[idx] - cum0; ci = ct[idx - 1] - cum0;
            }
            if (valid && (risky(e, cj, cj * inv_const, dl_const, inv_const) || risky(e, ci, ci * inv_const, dl_const, inv_const))) unsure = true;
            int prev = __shfl_up(idx, 1, WAVE);
            if (lane == 0) prev = last_idx;
            const bool isnew = valid && idx != prev;
            const unsigned long long mk = __ballot(isnew);
            const int pos = base + __popcll(mk & ((1ull << lane) - 1ull));
            if (isnew && pos < MAXF) s_keep[pos] = idx;
            base += __popcll(mk);
            const int nv = ntar - t0 < WAVE ? ntar - t0 : WAVE;
            last_idx = __shfl(idx, nv - 1, WAVE);
        }
    }
    if (n - 1 > WAVE && last_idx != n - 1) {              // keep_last_point
        if (lane == 0 && base < MAXF) s_keep[base] = n - 1;
        base++;
    }
    return base;
}

// Round 4: the ego prediction from the host's table (mpcx_interaction_params.plan_*).  Once the predicted speed has saturated dl is the
// constant DT * MAX_SPEED; if the points before that (four from standstill with the stock constants) all stay in bucket 0 with their
// own, smaller dl -- then they do with the constant one too -- the bucket sequence of trajectory_full[tidx:] is the one the host
// resampled with the constant dl, i.e. the kept poses depend on tidx alone: their number, their disc centres and the run boxes are ONE
// read of row tidx (one memory round trip) instead of the resampling pass, the disc arithmetic and the box reductions.
// Returns whether the table applies to this ego; then na poses are in s_ego and the runs' boxes in s_box.
__device__ __forceinline__ bool ego_from_plan(const Ego &e, size_t prow, double (*s_ego)[4], double (*s_box)[4], int &na) {
    const mpcx_interaction_params &ip = e.ip;
    const int lane = e.lane;
    if (!(ip.plan_cnt && e.cumtab && ip.plan_dl == e.dl_const && ip.plan_steps == ip.pred_steps && ip.plan_radius == ip.radius && ip.plan_cap <= e.MAXF && ip.plan_cap <= WAVE))
        return false;
    const int cnt = ip.plan_cnt[prow];
    // the row's disc centres and boxes are requested together with its count (the table has plan_cap poses per row whatever the count is):
    // one memory round trip, not two
    const double *pd = ip.plan_disc + prow * (size_t)ip.plan_cap * 4;
    const int f0 = lane < 2 * ip.plan_cap ? lane : 0, f1 = lane + WAVE < 2 * ip.plan_cap ? lane + WAVE : 0;
    const double e0x = pd[2 * f0], e0y = pd[2 * f0 + 1], e1x = pd[2 * f1], e1y = pd[2 * f1 + 1];
    const double bxv = ip.plan_box[prow * (4 * NSEG) + (lane < 4 * NSEG ? lane : 0)];
    // lane i: has the predicted speed of point i reached MAX_SPEED?  (monotone in i for max_accel >= 0)
    const bool sat = !e.accel_phase || !(__dadd_rn(__dmul_rn(ip.max_accel, (double)(lane + 1)), e.v) < ip.max_speed);
    const unsigned long long sm = __ballot(sat);
    const int isat = sm ? (int)__ffsll((long long)sm) - 1 : WAVE;
    bool bad = false;
    if (lane < isat && lane < e.n) {       // points with their own dl: bucket 0 needs c_i < dl_i, with the table's error bound on the safe side
        const double r = __dadd_rn(__dmul_rn(ip.max_accel, (double)(lane + 1)), e.v);
        const double dli = __dmul_rn(ip.dt, r);
        const double ci = e.cumtab[e.tidx + lane] - e.cum0;
        bad = !(ci + e.marg < dli * (1.0 - 1e-12)) || !(dli > 0.0);
    }
    if (!(cnt > 0 && cnt <= ip.plan_cap && ip.max_accel >= 0.0 && isat < WAVE && !__ballot(bad))) return false;
    na = cnt;
    // lane f handles disc f & 1 of pose f >> 1 (and f + 64 likewise; plan_cap <= 64 poses)
    if (lane < 2 * na) { s_ego[lane >> 1][2 * (lane & 1)] = e0x; s_ego[lane >> 1][2 * (lane & 1) + 1] = e0y; }
    if (lane + WAVE < 2 * na) { s_ego[(lane + WAVE) >> 1][2 * (lane & 1)] = e1x; s_ego[(lane + WAVE) >> 1][2 * (lane & 1) + 1] = e1y; }
    if (lane < 4 * NSEG) (&s_box[0][0])[lane] = bxv;
    return true;
}

// The ego frames come from exactly one of: the plan table (from_plan: discs and boxes are in LDS already), the boundary search, the
// point-by-point scan over the fast sums -- each of the last two redone with np.cumsum's own sums where a bucket was too close to call.
// Returns the number of frames; but for from_plan their path indices are in s_keep.
__device__ __forceinline__ int ego_frames(const Ego &e, size_t prow, double (*s_ego)[4], double (*s_box)[4], bool &from_plan) {
    int na = 0;
    bool unsure = false;
    from_plan = !FORCE_EXACT && ego_from_plan(e, prow, s_ego, s_box, na);
    if (from_plan) return na;
    if (e.cumtab && e.n > WAVE && !below_max_speed(e, WAVE)) na = resample_by_search(e, unsure);
    else {
        if (e.cumtab) sums_from_table(e);
        else prefix_fast(e);
        __syncthreads();
        na = resample_by_scan<true>(e, unsure);
    }
    if (FORCE_EXACT) unsure = true;
    if (__ballot(unsure)) {
        __syncthreads();
        prefix_exact(e);
        na = resample_by_scan<false>(e, unsure);
    }
    return na;
}

// ego disc centres per kept pose
__device__ __forceinline__ void ego_discs(const Ego &e, const double *rcs, int na, double (*s_ego)[4]) {
    for (int f = e.lane; f < na; f += WAVE) {
        const int i = e.s_keep[f];
        const double px = e.rem[3 * i], py = e.rem[3 * i + 1], c = rcs[2 * i], s = rcs[2 * i + 1];
        pose_discs(e.ip, px, py, c, s, s_ego[f]);
    }
}

// collision_avoidance.py:107-119 on trajectory_full, then mpc_intersection.py:130-134: the cut length for a conflict at path point
// `at` = (hx, hy)
__device__ __forceinline__ int cut_index(const mpcx_interaction_params &ip, const double *path, size_t path_row, int len, int tidx, int at,
                                         double hx, double hy, int lane) {
    int cut = 0x7fffffff;
    if (ip.path_first_within) {
        // (hx, hy) IS path point `at`: the first point within 1 mm of it is a property of the path, tabulated by the host with
        // the reference's own expression (mpcx_interaction_params.path_first_within) -- no scan of the path up to the conflict
        cut = ip.path_first_within[path_row + at];
    } else {
        const Within within(0.001);
        // (hx, hy) IS path point `at`, so the first index within 1 mm cannot lie beyond it: scan [0, at]
        const int jend = at + 1 < len ? at + 1 : len;
        for (int j = lane; j < jend; j += WAVE)         // same decision as sqrt(dx*dx + dy*dy) <= 0.001, no sqrt on the bulk
            if (within(path[3 * j], path[3 * j + 1], hx, hy)) cut = j < cut ? j : cut;
        cut = wave_min_i(cut);
    }
    int cl = len;
    if (cut != 0x7fffffff) { cl = cut - ip.cutoff_margin; cl = cl > tidx + 1 ? cl : tidx + 1; }
    return cl;
}

// departure (mpcx_scene): which rows of the agent's window [off, off + cnt) are in the scene and not its own, as a bit per window offset.
// One load of a mask word per lane and a ballot (cnt <= 64; a larger window is beyond the launch's capacity); the number of obstacles is its
// population count.  Rows outside the pool count as absent, so nothing is read from there later.
__device__ __forceinline__ unsigned long long present_rows(const InterArgs &a, int p, int lane, int cnt, int off, int own) {
    const int r = off + lane;
    const bool in = lane < cnt && r >= 0 && r < a.n_rows;
    const int32_t gone = a.absent[in ? r : 0];          // clamped address, selected afterwards (n_rows >= 1: checked by the host)
    return __ballot(in && r != own && gone == 0);
}

// right of way (mpcx_precedence): which of those rows YIELD to the agent -- present, not its own, and with a precedence word larger than its
// own row's -- as a bit per window offset: a second ballot, one more word load per lane (the own row's word is one wave-uniform load).
// An agent without an own row (own outside the pool) has nobody yield to it.
__device__ __forceinline__ unsigned long long yielding_rows(const InterArgs &a, int lane, int cnt, int off, int own, unsigned long long present) {
    const int r = off + lane;
    const bool in = lane < cnt && r >= 0 && r < a.n_rows;
    const bool has_own = own >= 0 && own < a.n_rows;
    const int32_t w = a.prec[in ? r : 0], wo = a.prec[has_own ? own : 0];          // clamped addresses, selected afterwards
    return __ballot(in && has_own && w > wo) & present;
}
// ... by RANK in the list of present rows (bit o = the o-th present row yields), as first_row's candidates are numbered: <= MPCX_MAX_OBS bits
__device__ __forceinline__ unsigned yields_by_rank(unsigned long long present, unsigned long long yielding) {
    unsigned out = 0u;
    for (unsigned long long m = yielding; m; m &= m - 1) {
        const int k = __ffsll((long long)m) - 1;
        out |= 1u << __popcll(present & ((1ull << k) - 1ull));
    }
    return out;
}

// RETIRE: the closed loop with retirement at the goal (mpcx_retire).  A template parameter, not a null test, as predict_kernel<MAPPED>:
// the launch without retirement runs the code it ran before there was any.
// SCENE (with RETIRE only): departure (mpcx_scene).  The obstacle list is the list of PRESENT rows of the window, built once per agent, and
// first_row walks nobs = its length candidates' worth of rows: a window with departed cars is less work.  The other two instantiations
// are the code they were.
// PREC (with RETIRE and SCENE only): right of way (mpcx_precedence).  The present rows that yield to the agent are a second ballot, and
// first_row loads their candidates from the standing records instead of the predictions; nothing else reads an obstacle's prediction
// (earliest_pose and cut_index work from the hit's disc position and the agent's own path).  The other three are the code they were.
// The statements of the kernel are mpcx_interaction_kernel_body.h, included below as text.
template <bool RETIRE, bool SCENE = false, bool PREC = false>
__global__ __launch_bounds__(64, 5) void interaction_kernel(InterArgs a) {
    static_assert(!PREC || (RETIRE && SCENE), "precedence lives on a scene");
#define MPCX_INTERACTION_SIGHT 0
#include "mpcx_interaction_kernel_body.h"
#undef MPCX_INTERACTION_SIGHT
}

// Line of sight (mpcx_sight; on retirement and a scene only).  The agent's word of seen rows, written by sight_kernel just before, is ANDed
// onto the ballot of present rows: a row the agent cannot see is, for it and only for it, an absent row.  nobs, rows and yields follow from
// the word; nothing else changes.  A kernel template of its own on InterSightArgs, not a fourth flag of interaction_kernel: that template
// keeps its three parameters and InterArgs its fields, so the four existing kernels keep their names, their arguments and their code.
template <bool PREC>
__global__ __launch_bounds__(64, 5) void interaction_sight_kernel(InterSightArgs a) {
    constexpr bool RETIRE = true, SCENE = true;
#define MPCX_INTERACTION_SIGHT 1
#include "mpcx_interaction_kernel_body.h"
#undef MPCX_INTERACTION_SIGHT
}

// The right-of-way instantiations (predict_kernel<·, true, true>, interaction_kernel<true, true, true>) are compiled in a translation unit of
// their own, mpcx_interaction_prec.hip, so that mpcx_interaction.hip keeps the kernels it had.  Their launchers, defined there and called by
// mpcx_interaction.hip:
void launch_predict_stand(bool mapped, int lanes, hipStream_t st, const PredArgs &pa);
void launch_interaction_prec(int P, size_t lds, hipStream_t st, const InterArgs &ia);
// The line-of-sight kernels (interaction_sight_kernel<false / true>) likewise: mpcx_interaction_sight.hip.
void launch_interaction_sight(int P, size_t lds, hipStream_t st, const InterArgs &ia, const unsigned long long *sight, bool prec);

}  // namespace mpcx
