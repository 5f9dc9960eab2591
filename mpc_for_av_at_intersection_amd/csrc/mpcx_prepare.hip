// mpcx_prepare.hip -- reference window, warm-start rollout and plant update, batched.
//
// Replaces (paths relative to /root/reference/main):
//   lib/mpc.py:86-109   _calc_ref_trajectory      -> ref_window_kernel  (a run of T + 1 lanes per instance)
//   lib/trajectories.py:100-126 calc_nearest_index_in_direction (inside the above)
//   lib/mpc.py:112-126  _predict_motion            -> rollout_kernel     (a group of lanes per instance)
//   lib/simulation.py:35-47 Simulation.step + bicycle/main.py:28-41      -> plant_kernel / rollout
// Arithmetic follows the reference's operation order; products are kept un-fused (-ffp-contract is
// irrelevant to the window's gathers; the plant's Euler updates are fused multiply-adds, see plant_euler).
#include "mpcx_common.h"
#include "mpcx_predict_core.h"
#include <cmath>

namespace mpcx {

struct RefArgs {
    mpcx_mpc_params p;
    int B;
    const double *state, *path, *path_v;
    const int32_t *path_off, *path_len;
    double dl;
    int32_t *target_ind;
    double *xref;
    uint8_t *re;
    const double *ov;       // speeds of the previous linearisation pass (mpc.py:226-237, MAX_ITER > 1): row b at ov + b * ov_stride, or nullptr
    long ov_stride;
    const int32_t *bin_cnt, *keyslot;   // closed loop: the conflict search filed agent b as (key, slot) = keyslot[b]; its place in the QP work queue
    int32_t *order;                     // (keys descending) = number of agents with a larger key + slot.  nullptr: no queue order is built
    // closed loop: the conflict search ran the same nearest-index scan for this agent (same state, same path) from near[3b]; near[3b+1] /
    // [3b+2] = the largest / smallest of its three nearest indices or -1, near_tidx[b] = its answer.  nullptr: always scan
    const int32_t *near, *near_tidx;
    // the stop index of lib/mpc_with_speed.py:276-282 (set_trajectory_fromarray(trajectory_full, cutoff_idx)): the window runs over the
    // agent's WHOLE path and cv = v_ref, 0 from stop_idx[b] on -- unless stop_idx[b] == 999, the reference's "no stop" (:281), whatever
    // the length of the path.  nullptr: no stop index (then the host passes v_ref = 0, today's xref[2] without a profile)
    const int32_t *stop_idx;
    double v_ref;
    int32_t *len_seen;      // with a stop index: <- n, the length of this step's tmp_trajectory (the next conflict search's prev_cut_len), or nullptr
    // retirement (read by the RETIRE instantiation only, which needs `order`): done[b] != 0 = agent b has arrived; queue_len <- the number
    // of agents filed in this step's queue
    const int32_t *done;
    int32_t *queue_len;
};

// RETIRE: the closed loop with retirement at the goal (mpcx_retire) -- a template parameter, not a null test: the launch without
// retirement runs the code it ran before there was any
//
// A wavefront takes WIN_AGENTS consecutive agents, a workgroup PREP_WAVES wavefronts.  (Until this layout every agent had a wavefront of
// its own, which summed the 16 x 64 queue counters again -- 134 MB of L2 reads per launch for a 4-KB table -- and then used T + 1 of its
// 64 lanes.)  Three parts:
//  1. per agent, lane i = agent b0 + i: its scalars, its place in the queue order, the nearest-index hint;
//  2. the agents whose hint misses: calc_nearest_index_in_direction by the whole wavefront, one agent at a time;
//  3. the windows, floor(64 / (T + 1)) agents per pass, each on a run of T + 1 lanes of its own.
constexpr int PREP_WAVES = 4;
constexpr int WIN_AGENTS = 8;
static_assert(WIN_AGENTS <= WAVE, "one lane per agent in parts 1 and 2");
template <bool RETIRE>
__global__ __launch_bounds__(64 * PREP_WAVES) void ref_window_kernel(RefArgs a) {
    // s_first[q][k] = the place in the queue of the first agent with key k that counted in copy q of the bins: the agents with a larger
    // key (suffix sums over the bins) + those with the same key in a lower copy.  Built once per workgroup
    __shared__ int s_first[MPCX_ORDER_COPIES][MPCX_ORDER_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = a.p.T, W = T + 1;
    const int b0 = ((int)blockIdx.x * PREP_WAVES + wave) * WIN_AGENTS;
    const int nag = a.B - b0 < WIN_AGENTS ? a.B - b0 : WIN_AGENTS;       // agents of this wavefront (<= 0: none, it only keeps the barrier)
    // ---- part 1: lane i < nag holds agent b0 + i (the other lanes read agent 0 and write nothing)
    const bool own = lane < nag;
    const int b = own ? b0 + lane : 0;
    bool gone = !own;
    if constexpr (RETIRE) gone = gone || a.done[b] != 0;       // retired: no place in the order, no output, len_seen untouched
    const int off = a.path_off[b], n = a.path_len[b];
    const double x = a.state[4 * b], y = a.state[4 * b + 1], v = a.state[4 * b + 2];
    const int start = a.target_ind[b];
    // (everything an agent reads is asked for here, in front of the barrier: one round trip to memory instead of one per dependent step)
    const int ks = a.order ? a.keyslot[b] : 0;
    const int hs = a.near ? a.near[3 * b] : -1, hm = a.near ? a.near[3 * b + 1] : -1, hl = a.near ? a.near[3 * b + 2] : -1;
    const int hint = a.near ? a.near_tidx[b] : -1;
    const int stop_at = a.stop_idx ? a.stop_idx[b] : MPCX_NO_STOP;
    if (a.order) {
        static_assert(MPCX_ORDER_BINS == 64, "one bin per lane");
        if (wave == 0) {        // lane k holds bin k
            int cnt[MPCX_ORDER_COPIES], c = 0;
#pragma unroll
            for (int q = 0; q < MPCX_ORDER_COPIES; q++) { cnt[q] = a.bin_cnt[q * MPCX_ORDER_BINS + lane]; c += cnt[q]; }
            int sfx = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_down(sfx, d); sfx += lane + d < 64 ? o : 0; }
            // lane 0's suffix sum is the sum of all bins over all copies = the agents the conflict search filed = the length of this step's
            // queue.  The first wavefront of the launch leaves it for the solve
            if constexpr (RETIRE) { if (blockIdx.x == 0 && lane == 0) *a.queue_len = sfx; }
            int first = sfx - c;
#pragma unroll
            for (int q = 0; q < MPCX_ORDER_COPIES; q++) { s_first[q][lane] = first; first += cnt[q]; }
        }
        __syncthreads();
        if (!gone)              // ... then the slot the conflict search drew
            a.order[s_first[b % MPCX_ORDER_COPIES][(ks >> 24) & (MPCX_ORDER_BINS - 1)] + (ks & 0xFFFFFF)] = b;
    }
    // The three nearest points of path[start .. n) are those of the conflict search's scan over path[hs .. len) whenever this range lies
    // inside that one (start >= hs) and holds all three (the three smallest of a set are the three smallest of every subset that contains
    // them; ties go to the lower index in both; the answer is a function of their absolute indices): then the answer is the conflict
    // search's and the scan is skipped.  Else (an earlier start, a cut in front of one of the three, an ego that did not advance): scan.
    int s = -1;
    bool scan = false;
    if (!gone) {
        if (hm >= 0 && start >= hs && hl >= start && hm < n) s = hint;
        else scan = !(start < 0 || n <= 0);
    }
    // ---- part 2: the scans, wave-cooperative, under a wave-uniform condition
    for (unsigned long long todo = __ballot(scan); todo; todo &= todo - 1) {
        const int i = __ffsll((long long)todo) - 1;
        const int r = nearest_index_in_direction(a.path + 3 * (size_t)__shfl(off, i), __shfl(n, i), __shfl(start, i), __shfl(x, i), __shfl(y, i), lane);
        s = lane == i ? r : s;
    }
    int stop = 0x7fffffff;
    if (!gone) {
        a.target_ind[b] = s;
        stop = stop_at == MPCX_NO_STOP ? stop : stop_at;
        if (a.stop_idx && a.len_seen) a.len_seen[b] = n;
    }
    // ---- part 3: lane = (agent g of the pass, window point t)
    const int G = 64 / W;
    const int g = lane / W, t = lane - g * W;
    for (int base = 0; base < nag; base += G) {
        const int i = base + g;
        const bool on = g < G && i < nag;
        const int from = on ? i : 0;
        const bool skip = __shfl((int)gone, from) != 0;
        const int si = __shfl(s, from), ni = __shfl(n, from), oi = __shfl(off, from), stopi = __shfl(stop, from);
        const double vi = __shfl(v, from);
        if (!on || skip) continue;
        const int bi = b0 + i;
        const double *path = a.path + 3 * (size_t)oi;
        const double *pv = a.path_v ? a.path_v + (size_t)oi : nullptr;   // mpc_with_speed.py:103-104
        double *xr = a.xref + (size_t)bi * 4 * W;
        uint8_t *re = a.re + (size_t)bi * W;
        if (si < 0) {  // reference raised: leave a defined (zero) window, caller sees target_ind = -1
            xr[t] = 0; xr[W + t] = 0; xr[2 * W + t] = 0; xr[3 * W + t] = 0; re[t] = 0;
            continue;
        }
        // mpc.py:95-100: ov = max(v, 10/3.6); travel = cumsum(|ov|*dt); idx = min(rint(travel/dl) + s, n-1)
        // from the second of MAX_ITER linearisation passes on, ov = the previous pass's speeds (mpc.py:226-237)
        const double ov = vi > 10.0 / 3.6 ? vi : 10.0 / 3.6;
        const double step = __dmul_rn(fabs(ov), a.p.dt);
        const double *ovp = a.ov ? a.ov + (size_t)bi * a.ov_stride : nullptr;
        double travel = ovp ? __dmul_rn(fabs(ovp[0]), a.p.dt) : step;                       // np.cumsum: sequential adds
        for (int k = 1; k <= t; k++) travel = __dadd_rn(travel, ovp ? __dmul_rn(fabs(ovp[k]), a.p.dt) : step);
        long long idx = (long long)rint(__ddiv_rn(travel, a.dl)) + si;
        if (idx > ni - 1) idx = ni - 1;
        xr[0 * W + t] = path[3 * idx];
        xr[1 * W + t] = path[3 * idx + 1];
        xr[2 * W + t] = idx >= stopi ? 0.0 : (pv ? pv[idx] : a.v_ref);
        xr[3 * W + t] = path[3 * idx + 2];
        re[t] = (idx == ni - 1);
    }
}

// simulation.py:35-47 + bicycle/main.py:28-41.  The pieces of one step; plant_step puts them together for one lane, rollout_kernel
// spreads them over a group of lanes.  Both evaluate these very expressions.  An Euler update acc + rate * dt is ONE fused multiply-add:
// that is what hipcc's default contraction has always made of it here (HIP's __dadd_rn / __dmul_rn are plain operators that fuse after
// inlining), and the results are compared bit for bit with that.  It is written out, with contraction off for everything else, so that
// the grouping of the operations cannot change it
__device__ __forceinline__ double plant_tan(const mpcx_mpc_params &p, double delta) {          // tan of the clamped steering angle
    return tan(fmax(fmin(delta, p.max_steer), -p.max_steer));
}
__device__ __forceinline__ double plant_rate_xy(double v, double cs) {      // d/dt of x (cs = cos th) or y (cs = sin th)
#pragma clang fp contract(off)
    return v * cs;
}
__device__ __forceinline__ double plant_rate_th(const mpcx_mpc_params &p, double v, double tn) {      // d/dt of th
#pragma clang fp contract(off)
    return (v / p.L) * tn;
}
__device__ __forceinline__ double plant_euler(const mpcx_mpc_params &p, double acc, double rate) { return fma(rate, p.dt, acc); }
__device__ __forceinline__ double plant_speed(const mpcx_mpc_params &p, double v, double a) {      // the speed after a step
    return fmax(fmin(plant_euler(p, v, a), p.max_speed), p.min_speed);
}
__device__ __forceinline__ void plant_step(const mpcx_mpc_params &p, double &x, double &y, double &v, double &th,
                                           double a, double delta) {
    const double tn = plant_tan(p, delta);
    double s, c;
    sincos(th, &s, &c);
    x = plant_euler(p, x, plant_rate_xy(v, c));
    y = plant_euler(p, y, plant_rate_xy(v, s));
    th = plant_euler(p, th, plant_rate_th(p, v, tn));
    v = plant_speed(p, v, a);
}

struct RollArgs {
    mpcx_mpc_params p;
    int B;
    const double *state, *u_warm;
    double *xbar;
    const int32_t *done;    // retirement (read by the RETIRE instantiation only): the row of an agent with done[b] != 0 is neither computed nor written
};

// Rollout of ROLL_AGENTS instances by one workgroup, a group of ROLL_GROUP lanes per instance, lane j of it the steps t = j, j + ROLL_GROUP,
// ...: of plant_step's recurrence only the running values v_t (with its clamp), th_t, x_t, y_t are serial (group_chain: every lane of the
// group walks them in step order); tan of the steering input, the divide in th's increment, sincos(th_t) and the products in x's and
// y's increments are evaluated once, by the step's own lane.  (One lane per instance walked T dependent sincos + tan + divide: 29 us
// beside the conflict search, which it cost 7 us.)  Results are staged in LDS and written as ONE contiguous run: the instances' xbar rows
// are adjacent in memory (ROLL_AGENTS x 4 x (T+1) doubles); straight from the lanes they would be 8-byte stores at four strides.  The
// staging buffer is dynamic LDS sized for the horizon in use: 43.5 KB at T = 20, 68 KB at T = 32, as much as one lane per instance
// needed for its 64 instances.  Groups of 4 measured 20.1 us, of 8 26.7, of 16 109, of 32 195: every lane walks the whole chain.
// RETIRE: a retired agent's xbar row stays as its last driven step left it (its state and inputs are frozen, so the row would come out
// the same from the step after its arrival on -- but not the same as that last driven step's, which started one state earlier)
constexpr int ROLL_GROUP = 4, ROLL_BLOCK = 256, ROLL_AGENTS = ROLL_BLOCK / ROLL_GROUP;
static_assert(WAVE % ROLL_GROUP == 0 && ROLL_BLOCK % WAVE == 0, "whole groups per wavefront");
inline size_t rollout_lds(int T) { return ROLL_AGENTS * (4 * (size_t)(T + 1) + 1) * sizeof(double); }
// one agent's rollout from (x, y, v, th) by its group of lanes (j = the lane's place in the group) into its staging row xb[4 W];
// oa = its warm start (T accelerations | T steering angles) or nullptr = zeros
__device__ __forceinline__ void rollout_group(const mpcx_mpc_params &p, double x, double y, double v, double th, const double *oa, int j, double *xb) {
    constexpr int G = ROLL_GROUP;
    const int T = p.T, W = T + 1;
    if (j == 0) { xb[0] = x; xb[W] = y; xb[2 * W] = v; xb[3 * W] = th; }
    const auto euler = [&](double acc, double rate) { return plant_euler(p, acc, rate); };
    const auto speed = [&](double vv, double acc) { return plant_speed(p, vv, acc); };
    // x, y, v, th: the state at step t0, the same in every lane of the group; lane j takes the step from t = t0 + j to t + 1
    for (int t0 = 0; t0 < T; t0 += G) {
        const int t = t0 + j;
        const bool in = t < T;
        const double ai = oa && in ? oa[t] : 0.0, di = oa && in ? oa[T + t] : 0.0;   // mpc.py:222-224: zeros when no warm start
        const double tn = plant_tan(p, di);
        const double v0 = v, th0 = th;
        const double vn = group_chain<G>(v, ai, j, speed);                  // v_{t+1}
        const double vt = group_prev<G>(vn, v0, j);                         // v_t
        const double thn = group_chain<G>(th, plant_rate_th(p, vt, tn), j, euler);
        const double tht = group_prev<G>(thn, th0, j);
        double s, c;
        sincos(tht, &s, &c);
        const double xn = group_chain<G>(x, plant_rate_xy(vt, c), j, euler);
        const double yn = group_chain<G>(y, plant_rate_xy(vt, s), j, euler);
        if (in) { xb[t + 1] = xn; xb[W + t + 1] = yn; xb[2 * W + t + 1] = vn; xb[3 * W + t + 1] = thn; }
    }
}
template <bool RETIRE>
__global__ __launch_bounds__(ROLL_BLOCK) void rollout_kernel(RollArgs a) {
    constexpr int G = ROLL_GROUP;
    extern __shared__ double s_roll[];                   // [ROLL_AGENTS][4 W + 1]; +1: rows of 4 W doubles would share their banks; it holds the row's "retired" flag
    const int T = a.p.T, W = T + 1;
    const int RS = 4 * W + 1;
    auto s_x = [&](int row) -> double * { return s_roll + (size_t)row * RS; };
    const int b0 = (int)blockIdx.x * ROLL_AGENTS;
    const int n = a.B - b0 < ROLL_AGENTS ? a.B - b0 : ROLL_AGENTS;
    const int r = (int)threadIdx.x / G, j = (int)threadIdx.x % G;
    bool gone = r >= n;
    if constexpr (RETIRE) gone = gone || a.done[b0 + r] != 0;
    if (j == 0) s_x(r)[4 * W] = gone ? 1.0 : 0.0;
    if (!gone) {            // (the same for every lane of a group)
        const int b = b0 + r;
        double x = a.state[4 * b], y = a.state[4 * b + 1], v = a.state[4 * b + 2], th = a.state[4 * b + 3];
        rollout_group(a.p, x, y, v, th, a.u_warm ? a.u_warm + (size_t)b * 2 * T : nullptr, j, s_x(r));
    }
    __syncthreads();
    double *out = a.xbar + (size_t)b0 * 4 * W;
    for (int i = threadIdx.x; i < n * 4 * W; i += ROLL_BLOCK) {
        const int row = i / (4 * W);
        if (!RETIRE || s_x(row)[4 * W] == 0.0) out[i] = s_x(row)[i - row * 4 * W];
    }
}

// The two halves of mpc.py:211-239's preparation are independent and run BESIDE each other: the rollout on the context's side stream
// (fork / join by events, capturable into the closed loop's hipGraph), the window selection on the context's stream.  (Until round 3 both
// were workgroups of one launch; the rollout's staging buffer would have been allocated for every workgroup of it.)

struct PlantArgs {
    mpcx_mpc_params p;
    int B;
    double *state;
    double *u;
    const int32_t *status;
    double *applied;
    const mpcx_qp_tuning *tune;   // per-instance MAX_DECEL or nullptr
    const int32_t *iters;         // closed loop only: the solver's iteration counts ...
    unsigned long long *stats;    // ... and the run statistics they are added to: agent-steps, iterations, failed solves, max iterations
    int has_stats;
    int32_t *zero_bins, *zero_ticket;   // closed loop: the queue bins and the ticket are zeroed for the next step (nullptr otherwise)
    const int32_t *done;                // retirement or nullptr: the lane of an agent with done[b] != 0 leaves state, applied and u alone and feeds no statistics
};

// the run statistics of the 64 agents of one wavefront (lane = agent b; in: it drove this step, it = its iteration count, bad: its solve
// failed) are added to the wavefront's slot, b / 64
__device__ __forceinline__ void plant_stats(unsigned long long *stats, int b, bool in, int it, bool bad) {
    int s_it = it, s_bad = bad ? 1 : 0, s_n = in ? 1 : 0, s_mx = it;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s_it += __shfl_xor(s_it, d, WAVE); s_bad += __shfl_xor(s_bad, d, WAVE); s_n += __shfl_xor(s_n, d, WAVE);
        const int o = __shfl_xor(s_mx, d, WAVE); s_mx = o > s_mx ? o : s_mx;
    }
    if ((threadIdx.x & 63) == 0) {
        // one slot of four counters per wavefront, touched by that wavefront only (steps are ordered by the stream): no atomics --
        // 2048 atomics on four hot words made this 5-us kernel a 22-us one
        unsigned long long *w = stats + 4 * (size_t)(b >> 6);
        w[0] += (unsigned long long)s_n; w[1] += (unsigned long long)s_it; w[2] += (unsigned long long)s_bad;
        if ((unsigned long long)s_mx > w[3]) w[3] = (unsigned long long)s_mx;
    }
}

// MPC.step's tail (mpc.py:294-297) + Simulation.step
__global__ __launch_bounds__(256) void plant_kernel(PlantArgs a) {
    if (a.zero_bins && blockIdx.x == 0) {
        for (int i = threadIdx.x; i < MPCX_ORDER_COPIES * MPCX_ORDER_BINS; i += blockDim.x) a.zero_bins[i] = 0;
        if (threadIdx.x < MPCX_TICKET_WORDS) a.zero_ticket[threadIdx.x] = 0;
    }
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const bool gone = a.done && b < a.B && a.done[b] != 0;
    if (a.has_stats) {          // run statistics (mpcx_closed_loop_stats)
        const bool in = b < a.B && !gone;
        plant_stats(a.stats, b, in, in ? a.iters[b] : 0, in && a.status[b] != MPCX_QP_OPTIMAL);
    }
    if (b >= a.B || gone) return;
    const int T = a.p.T;
    double di = a.applied[2 * b], ai;
    const bool ok = !a.status || a.status[b] == MPCX_QP_OPTIMAL;
    if (ok) { di = a.u[(size_t)b * 2 * T + T]; ai = a.u[(size_t)b * 2 * T]; }
    else {
        ai = a.tune ? a.tune[b].max_decel : a.p.max_decel;
        for (int t = 0; t < 2 * T; t++) a.u[(size_t)b * 2 * T + t] = 0.0;   // warm start reset, mpc.py:222-224
    }
    a.applied[2 * b] = di; a.applied[2 * b + 1] = ai;
    double x = a.state[4 * b], y = a.state[4 * b + 1], v = a.state[4 * b + 2], th = a.state[4 * b + 3];
    plant_step(a.p, x, y, v, th, ai, di);
    a.state[4 * b] = x; a.state[4 * b + 1] = y; a.state[4 * b + 2] = v; a.state[4 * b + 3] = th;
}

struct HeadArgs {
    mpcx_mpc_params p;
    mpcx_interaction_params ip;
    int B;
    double *state, *applied, *u;      // u: the previous solution, the rollout's warm start
    double *xbar, *obs6, *pred;       // the pool (row q = agent q) and the prediction scratch [B][pred_steps][2][2]
    // PLANT only: what plant_kernel gets (PlantArgs) for the step before
    const int32_t *status, *iters;
    const mpcx_qp_tuning *tune;
    unsigned long long *stats;
    int32_t *zero_bins, *zero_ticket;
};

// The head of a closed-loop step in ONE launch: what belongs to agent q alone and reads nothing but q's own state, applied inputs and
// previous solution -- the plant update of the step before (PLANT; plant_kernel), the pack and the prediction of pool row q
// (predict_kernel<false>) and the warm-start rollout of agent q (rollout_kernel<false>).  The rollout is over before the conflict search
// starts: no side stream, no fork, no join, and one dependent launch boundary instead of two.
// A workgroup takes ROLL_AGENTS = 64 agents: wavefronts 0..3 are rollout_kernel's workgroup (a group of ROLL_GROUP lanes per agent), wavefront
// 4 is predict_kernel's and plant_kernel's wavefront (a lane per agent).  The two serial chains (pred_steps dependent sincos, T / ROLL_GROUP
// chain steps) sit in different wavefronts and run beside each other.  PLANT: EVERY lane takes its agent's plant step in registers (one tan,
// one sincos) from the old state; the lanes of wavefront 4 alone store state, applied, the reset warm start and the statistics -- behind
// the workgroup's one barrier, in front of which every lane has loaded what it needs of the old values.  A rollout group whose agent's
// solve failed takes zeros for the warm start that wavefront 4 resets: it never loads it.  No workgroup waits for another.
// Every wavefront of the rollout writes its own 16 agents' rows to LDS and copies them out itself (one contiguous run of 16 x 4 W doubles):
// it waits for nobody, wavefront 4's chain included.
constexpr int HEAD_BLOCK = ROLL_BLOCK + WAVE;
static_assert(ROLL_AGENTS == WAVE, "the prediction wavefront holds the workgroup's agents one per lane; its statistics slot is plant_kernel's");
template <bool PLANT>
__global__ __launch_bounds__(HEAD_BLOCK) void head_kernel(HeadArgs a) {
    constexpr int G = ROLL_GROUP;
    extern __shared__ double s_roll[];                   // [ROLL_AGENTS][4 W + 1], rollout_kernel's rows (the spare word keeps them off each other's banks)
    const int T = a.p.T, W = T + 1;
    const int RS = 4 * W + 1;
    const int tid = (int)threadIdx.x;
    const bool pred_wave = tid >= ROLL_BLOCK;
    const int b0 = (int)blockIdx.x * ROLL_AGENTS;
    const int n = a.B - b0 < ROLL_AGENTS ? a.B - b0 : ROLL_AGENTS;
    const int r = pred_wave ? tid - ROLL_BLOCK : tid / G, j = tid % G;
    const bool in = r < n;
    const int b = b0 + (in ? r : 0);        // (the lanes without an agent read the workgroup's first and write nothing)
    double x = a.state[4 * b], y = a.state[4 * b + 1], v = a.state[4 * b + 2], th = a.state[4 * b + 3];
    double di = 0.0, ai = 0.0;              // the inputs applied to reach (x, y, v, th): (steer, accel)
    bool failed = false;
    if constexpr (PLANT) {
        if (a.zero_bins && blockIdx.x == 0) {
            for (int i = tid; i < MPCX_ORDER_COPIES * MPCX_ORDER_BINS; i += HEAD_BLOCK) a.zero_bins[i] = 0;
            if (tid < MPCX_TICKET_WORDS) a.zero_ticket[tid] = 0;
        }
        // plant_kernel's expressions for the step before, in every lane
        failed = a.status[b] != MPCX_QP_OPTIMAL;
        const int it = pred_wave && in ? a.iters[b] : 0;
        di = a.applied[2 * b];
        if (!failed) { di = a.u[(size_t)b * 2 * T + T]; ai = a.u[(size_t)b * 2 * T]; }
        else { ai = a.p.max_decel; if (a.tune) ai = a.tune[b].max_decel; }      // (as a ?: of the two the kernel argument went to a stack slot)
        plant_step(a.p, x, y, v, th, ai, di);
        __syncthreads();        // every lane holds what it needs of the old state, applied and u: now they may be overwritten
        if (pred_wave) {
            plant_stats(a.stats, b0 + r, in, it, in && failed);
            if (in) {
                if (failed) for (int t = 0; t < 2 * T; t++) a.u[(size_t)b * 2 * T + t] = 0.0;   // warm start reset, mpc.py:222-224
                a.applied[2 * b] = di; a.applied[2 * b + 1] = ai;
                a.state[4 * b] = x; a.state[4 * b + 1] = y; a.state[4 * b + 2] = v; a.state[4 * b + 3] = th;
            }
        }
    } else if (pred_wave) {
        di = a.applied[2 * b]; ai = a.applied[2 * b + 1];
    }
    if (pred_wave) {
        if (!in) return;
        // predict_kernel<false> with the pool pack: MovingObstacle*.get() = (x, y, v, yaw, a, steer)
        double *row = a.obs6 + 6 * (size_t)b;
        row[0] = x; row[1] = y; row[2] = v; row[3] = th; row[4] = ai; row[5] = di;
        predict_row<false>(a.ip, x, y, v, th, ai, di, nullptr, a.pred + (size_t)b * a.ip.pred_steps * 4);
        return;
    }
    if (in) rollout_group(a.p, x, y, v, th, failed ? nullptr : a.u + (size_t)b * 2 * T, j, s_roll + (size_t)r * RS);
    // the rows of this wavefront's agents were written by its own lanes: LDS serves a wavefront's accesses in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    constexpr int ROWS = WAVE / G;
    const int lane = tid & 63, r0 = (tid >> 6) * ROWS;
    const int nr = n - r0 < ROWS ? n - r0 : ROWS;       // (<= 0: a wavefront without agents)
    double *out = a.xbar + (size_t)(b0 + r0) * 4 * W;
    for (int i = lane; i < nr * 4 * W; i += WAVE) {
        const int row = i / (4 * W);
        out[i] = s_roll[(size_t)(r0 + row) * RS + (i - row * 4 * W)];
    }
}

}  // namespace mpcx

extern "C" int32_t mpcx_mpc_prepare_batch(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm,
                                          const double *path_xyyaw, const double *path_v, const int32_t *path_off,
                                          const int32_t *path_len, double dl, int32_t *target_ind, double *xref, uint8_t *reaches_end, double *xbar) {
    return mpcx_mpc_prepare_batch_ov(ctx, B, state, u_warm, path_xyyaw, path_v, path_off, path_len, dl, target_ind, nullptr, 0, xref, reaches_end, xbar);
}

extern "C" int32_t mpcx_mpc_prepare_batch_ov(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm,
                                             const double *path_xyyaw, const double *path_v, const int32_t *path_off,
                                             const int32_t *path_len, double dl, int32_t *target_ind, const double *ov, int64_t ov_stride,
                                             double *xref, uint8_t *reaches_end, double *xbar) {
    return mpcx_window_enqueue(ctx, B, state, u_warm, path_xyyaw, path_v, path_off, path_len, dl, target_ind, ov, ov_stride, xref, reaches_end, xbar, {});
}

extern "C" int32_t mpcx_mpc_prepare_batch_stop(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm,
                                               const double *path_xyyaw, const double *path_v, const int32_t *path_off,
                                               const int32_t *path_len, double dl, int32_t *target_ind, const double *ov, int64_t ov_stride,
                                               const int32_t *stop_idx, double v_ref, int32_t *len_seen,
                                               double *xref, uint8_t *reaches_end, double *xbar) {
    mpcx_window_extras wx;
    wx.stop_idx = stop_idx; wx.v_ref = v_ref; wx.len_seen = len_seen;
    return mpcx_window_enqueue(ctx, B, state, u_warm, path_xyyaw, path_v, path_off, path_len, dl, target_ind, ov, ov_stride, xref, reaches_end, xbar, wx);
}

int32_t mpcx_window_enqueue(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm, const double *path_xyyaw, const double *path_v,
                            const int32_t *path_off, const int32_t *path_len, double dl, int32_t *target_ind, const double *ov, int64_t ov_stride,
                            double *xref, uint8_t *reaches_end, double *xbar, const mpcx_window_extras &x) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (B == 0) return MPCX_OK;       // empty batch: nothing to do (zero-size tensors have null data pointers)
    if (B < 0 || !state || !path_xyyaw || !path_off || !path_len || !target_ind || !xref || !reaches_end || !xbar || !(dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "mpc_prepare_batch: null pointer, negative batch or dl <= 0");
    if (ov && ov_stride < (int64_t)ctx->mpc.T + 1)
        return mpcx_fail(ctx, MPCX_E_INVALID, "mpc_prepare_batch_ov: ov_stride %lld is smaller than T + 1", (long long)ov_stride);
    if (x.stop_idx && !std::isfinite(x.v_ref))
        return mpcx_fail(ctx, MPCX_E_INVALID, "mpc_prepare_batch_stop: v_ref is not finite");
    mpcx::RefArgs ra{ctx->mpc, B, state, path_xyyaw, path_v, path_off, path_len, dl, target_ind, xref, reaches_end, ov, (long)ov_stride,
                     x.scatter ? ctx->bins : nullptr, x.scatter ? ctx->bins + MPCX_ORDER_COPIES * MPCX_ORDER_BINS : nullptr, x.scatter ? ctx->order : nullptr,
                     x.near, x.near ? x.tidx : nullptr, x.stop_idx, x.stop_idx ? x.v_ref : 0.0, x.stop_idx ? x.len_seen : nullptr,
                     x.done, x.queue_len};
    const bool retire = x.done != nullptr;
    if (retire && (!x.scatter || !x.queue_len))
        return mpcx_fail(ctx, MPCX_E_INVALID, "mpc_prepare_batch: retirement needs the queue order built beside the window selection");
    // the rollout may already be in flight: mpcx_closed_loop_run forks it at the start of the step, beside the conflict search
    const bool forked = x.rollout_forked;
    if (x.rollout_done) {       // xbar is written already, by a launch in front of this one on the context's stream: no side stream, no events
        constexpr int per_block = mpcx::PREP_WAVES * mpcx::WIN_AGENTS;
        const dim3 wgrid((B + per_block - 1) / per_block), wblock(64 * mpcx::PREP_WAVES);
        if (retire) hipLaunchKernelGGL(mpcx::ref_window_kernel<true>, wgrid, wblock, 0, ctx->stream, ra);
        else hipLaunchKernelGGL(mpcx::ref_window_kernel<false>, wgrid, wblock, 0, ctx->stream, ra);
        return mpcx_check_launch(ctx, "prepare kernels");
    }
    if (!forked) {
        int32_t rc = mpcx_rollout_fork(ctx, B, state, u_warm, xbar, x.done);
        if (rc != MPCX_OK) return rc;
    }
    // a rollout forked long ago (mpcx_closed_loop_run: at the start of the step) is joined IN FRONT of the window selection: the queue
    // works the barrier off while the conflict search is still running, and nothing stands between the window kernel and the solve;
    // a rollout forked just now runs beside the window selection and is joined behind it
    if (forked && hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "mpc_prepare_batch: cannot join the side stream");
    constexpr int per_block = mpcx::PREP_WAVES * mpcx::WIN_AGENTS;
    const dim3 wgrid((B + per_block - 1) / per_block), wblock(64 * mpcx::PREP_WAVES);
    if (retire) hipLaunchKernelGGL(mpcx::ref_window_kernel<true>, wgrid, wblock, 0, ctx->stream, ra);
    else hipLaunchKernelGGL(mpcx::ref_window_kernel<false>, wgrid, wblock, 0, ctx->stream, ra);
    if (!forked && hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "mpc_prepare_batch: cannot join the side stream");
    return mpcx_check_launch(ctx, "prepare kernels");
}

// the warm-start rollout (mpc.py:112-126 `_predict_motion`) on the context's side stream, ordered behind everything enqueued on the
// context's stream so far; mpcx_window_enqueue joins it (mpcx_window_extras::rollout_forked: instead of forking one of its own)
int32_t mpcx_rollout_fork(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm, double *xbar, const int32_t *done) {
    mpcx::RollArgs ro{ctx->mpc, B, state, u_warm, xbar, done};
    if (hipEventRecord(ctx->ev_fork, ctx->stream) != hipSuccess || hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "mpc_prepare_batch: cannot fork the side stream");
    const size_t roll_lds = mpcx::rollout_lds(ctx->mpc.T);
    const dim3 rgrid((B + mpcx::ROLL_AGENTS - 1) / mpcx::ROLL_AGENTS), rblock(mpcx::ROLL_BLOCK);
    if (done) hipLaunchKernelGGL(mpcx::rollout_kernel<true>, rgrid, rblock, roll_lds, ctx->side, ro);
    else hipLaunchKernelGGL(mpcx::rollout_kernel<false>, rgrid, rblock, roll_lds, ctx->side, ro);
    // a refused launch is the rollout's failure, not that of whichever call checks the error state next
    const int32_t rc = mpcx_check_launch(ctx, "rollout_kernel");
    if (rc != MPCX_OK) return rc;
    // the join event right behind the rollout: by the time the context's stream waits for it (in front of the solve) the marker has long
    // been processed -- recorded there, the wait paid for the side queue's marker AND its own barrier
    if (hipEventRecord(ctx->ev_join, ctx->side) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "mpc_prepare_batch: cannot record the join event");
    return MPCX_OK;
}

// the head of a closed-loop step (head_kernel): plant = it also takes the plant step of the step before, with the statistics, and -- reset_bins --
// zeroes the queue bins and the ticket, as mpcx_plant_enqueue would have.  Local pool without scripted traffic only: obs6 row q is agent q
int32_t mpcx_head_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, double *state, double *applied, double *u,
                          const int32_t *status, const int32_t *iters, double *xbar, double *obs6, bool plant, bool reset_bins) {
    if (!ctx || !ip || P <= 0 || !state || !applied || !u || !status || !iters || !xbar || !obs6 || !ctx->pred || !ctx->stats)
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: null pointer at the head of a step");
    if (ctx->pred_cap < (size_t)P * ip->pred_steps * 4 * sizeof(double) || ctx->stats_slots < ((size_t)P + 63) / 64)
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: the prediction scratch or the statistics are too small for %d agents", P);
    if (ctx->tune && ctx->tune_rows != P)
        return mpcx_fail(ctx, MPCX_E_INVALID, "plant_step_batch: %d tuning rows are set but the batch has %d agents", ctx->tune_rows, P);
    const bool rz = plant && reset_bins && ctx->bins && ctx->ticket;
    mpcx::HeadArgs ha{ctx->mpc, *ip, P, state, applied, u, xbar, obs6, ctx->pred, status, iters, ctx->tune, ctx->stats,
                      rz ? ctx->bins : nullptr, rz ? ctx->ticket : nullptr};
    const size_t lds = mpcx::rollout_lds(ctx->mpc.T);
    const dim3 grid((P + mpcx::ROLL_AGENTS - 1) / mpcx::ROLL_AGENTS), block(mpcx::HEAD_BLOCK);
    if (plant) hipLaunchKernelGGL(mpcx::head_kernel<true>, grid, block, lds, ctx->stream, ha);
    else hipLaunchKernelGGL(mpcx::head_kernel<false>, grid, block, lds, ctx->stream, ha);
    return mpcx_check_launch(ctx, "head_kernel");
}

extern "C" int32_t mpcx_plant_step_batch(mpcx_ctx *ctx, int32_t B, double *state, double *u,
                                         const int32_t *status, double *applied) {
    return mpcx_plant_enqueue(ctx, B, state, u, status, applied, {});
}

int32_t mpcx_plant_enqueue(mpcx_ctx *ctx, int32_t B, double *state, double *u, const int32_t *status, double *applied, const mpcx_plant_extras &x) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (B == 0) return MPCX_OK;       // empty batch: nothing to do (zero-size tensors have null data pointers)
    if (B < 0 || !state || !u || !applied) return mpcx_fail(ctx, MPCX_E_INVALID, "plant_step_batch: null pointer");
    if (ctx->tune && ctx->tune_rows != B)
        return mpcx_fail(ctx, MPCX_E_INVALID, "plant_step_batch: %d tuning rows are set but the batch has %d agents", ctx->tune_rows, B);
    const bool st = ctx->stats && x.stats_iters && status;
    const bool rz = x.reset_bins && ctx->bins && ctx->ticket;
    mpcx::PlantArgs pa{ctx->mpc, B, state, u, status, applied, ctx->tune, x.stats_iters, ctx->stats, st ? 1 : 0,
                       rz ? ctx->bins : nullptr, rz ? ctx->ticket : nullptr, x.done};
    hipLaunchKernelGGL(mpcx::plant_kernel, dim3((B + 63) / 64), dim3(64), 0, ctx->stream, pa);
    return mpcx_check_launch(ctx, "plant_kernel");
}

extern "C" int32_t mpcx_closed_loop_stats(mpcx_ctx *ctx, int64_t *out4, int32_t reset) {
    if (!ctx || !out4) return MPCX_E_INVALID;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!ctx->stats || !ctx->stats_slots) return MPCX_OK;
    std::vector<unsigned long long> h(4 * ctx->stats_slots);
    if (hipMemcpyAsync(h.data(), ctx->stats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_stats: copy failed");
    for (size_t w = 0; w < ctx->stats_slots; w++) {
        out4[0] += (int64_t)h[4 * w]; out4[1] += (int64_t)h[4 * w + 1]; out4[2] += (int64_t)h[4 * w + 2];
        if ((int64_t)h[4 * w + 3] > out4[3]) out4[3] = (int64_t)h[4 * w + 3];
    }
    if (reset && hipMemsetAsync(ctx->stats, 0, h.size() * sizeof(unsigned long long), ctx->stream) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_stats: reset failed");
    return MPCX_OK;
}

extern "C" int32_t mpcx_closed_loop_queue(mpcx_ctx *ctx, int32_t P, int32_t *order, int32_t *keyslot) {
    if (!ctx || !order || !keyslot || P < 0) return MPCX_E_INVALID;
    const size_t counters = (size_t)MPCX_ORDER_COPIES * MPCX_ORDER_BINS;
    if (!ctx->order || !ctx->bins || ctx->order_cap < (size_t)P * sizeof(int32_t) || ctx->bins_cap < (counters + (size_t)P) * sizeof(int32_t))
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_queue: no closed loop has built a work queue for %d agents on this context", P);
    if (P == 0) return MPCX_OK;
    if (hipMemcpyAsync(order, ctx->order, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(keyslot, ctx->bins + counters, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_queue: copy failed");
    return MPCX_OK;
}
