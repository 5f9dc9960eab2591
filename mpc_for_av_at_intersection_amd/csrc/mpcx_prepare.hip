// mpcx_prepare.hip -- reference window, warm-start rollout and plant update, batched.
//
// Replaces (paths relative to /root/reference/main):
//   lib/mpc.py:86-109   _calc_ref_trajectory      -> ref_window_kernel  (one wavefront per instance)
//   lib/trajectories.py:100-126 calc_nearest_index_in_direction (inside the above)
//   lib/mpc.py:112-126  _predict_motion            -> rollout_kernel     (one thread per instance)
//   lib/simulation.py:35-47 Simulation.step + bicycle/main.py:28-41      -> plant_kernel / rollout
// Arithmetic follows the reference's operation order; products are kept un-fused (-ffp-contract is
// irrelevant here because every product/sum below goes through __dmul_rn/__dadd_rn where order matters).
#include "mpcx_common.h"
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
template <bool RETIRE>
__device__ __forceinline__ void ref_window_block(const RefArgs &a, int b) {
    const int lane = threadIdx.x & 63;
    const int T = a.p.T, W = T + 1;
    if (a.order) {
        // lane k holds bin k.  Agents with a larger key come first (suffix sums over the bins by shuffles), then the agents of the same key
        // that counted in a lower copy of the bins, then the slot the conflict search drew
        static_assert(MPCX_ORDER_BINS == 64, "one bin per lane");
        const int mine = b % MPCX_ORDER_COPIES;
        int c = 0, lower = 0;
#pragma unroll
        for (int q = 0; q < MPCX_ORDER_COPIES; q++) {
            const int v = a.bin_cnt[q * MPCX_ORDER_BINS + lane];
            c += v;
            lower += q < mine ? v : 0;
        }
        int sfx = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_down(sfx, d); sfx += lane + d < 64 ? o : 0; }
        if constexpr (RETIRE) {
            // lane 0's suffix sum is the sum of all bins over all copies = the agents the conflict search filed = the length of this step's
            // queue.  The first wavefront of the launch leaves it for the solve, whether its own agent is retired or not
            if (b == 0 && lane == 0) *a.queue_len = sfx;
            if (a.done[b] != 0) return;       // retired: no place in the order, no output, len_seen untouched
        }
        const int ks = a.keyslot[b];
        const int first = __shfl(sfx - c + lower, ks >> 24);
        if (lane == 0) a.order[first + (ks & 0xFFFFFF)] = b;
    }
    const double *path = a.path + 3 * (size_t)a.path_off[b];
    const double *pv = a.path_v ? a.path_v + (size_t)a.path_off[b] : nullptr;   // mpc_with_speed.py:103-104
    const int n = a.path_len[b];
    const double x = a.state[4 * b], y = a.state[4 * b + 1], v = a.state[4 * b + 2];
    int start = a.target_ind[b];
    // The three nearest points of path[start .. n) are those of the conflict search's scan over path[hs .. len) whenever this range lies
    // inside that one (start >= hs) and holds all three (the three smallest of a set are the three smallest of every subset that contains
    // them; ties go to the lower index in both; the answer is a function of their absolute indices): then the answer is the conflict
    // search's and the scan is skipped.  Else (an earlier start, a cut in front of one of the three, an ego that did not advance): scan.
    int s;
    const int hs = a.near ? a.near[3 * b] : -1, hm = a.near ? a.near[3 * b + 1] : -1, hl = a.near ? a.near[3 * b + 2] : -1;
    if (hm >= 0 && start >= hs && hl >= start && hm < n) s = a.near_tidx[b];
    else s = (start < 0 || n <= 0) ? -1 : nearest_index_in_direction(path, n, start, x, y, lane);
    if (lane == 0) a.target_ind[b] = s;
    int stop = 0x7fffffff;
    if (a.stop_idx) {
        const int c = a.stop_idx[b];
        stop = c == MPCX_NO_STOP ? stop : c;
        if (a.len_seen && lane == 0) a.len_seen[b] = n;
    }
    double *xr = a.xref + (size_t)b * 4 * W;
    uint8_t *re = a.re + (size_t)b * W;
    if (s < 0) {  // reference raised: leave a defined (zero) window, caller sees target_ind = -1
        if (lane <= T) { xr[lane] = 0; xr[W + lane] = 0; xr[2 * W + lane] = 0; xr[3 * W + lane] = 0; re[lane] = 0; }
        return;
    }
    // mpc.py:95-100: ov = max(v, 10/3.6); travel = cumsum(|ov|*dt); idx = min(rint(travel/dl) + s, n-1)
    // from the second of MAX_ITER linearisation passes on, ov = the previous pass's speeds (mpc.py:226-237)
    const double ov = v > 10.0 / 3.6 ? v : 10.0 / 3.6;
    const double step = __dmul_rn(fabs(ov), a.p.dt);
    const double *ovp = a.ov ? a.ov + (size_t)b * a.ov_stride : nullptr;
    if (lane <= T) {
        double travel = ovp ? __dmul_rn(fabs(ovp[0]), a.p.dt) : step;                       // np.cumsum: sequential adds
        for (int k = 1; k <= lane; k++) travel = __dadd_rn(travel, ovp ? __dmul_rn(fabs(ovp[k]), a.p.dt) : step);
        long long idx = (long long)rint(__ddiv_rn(travel, a.dl)) + s;
        if (idx > n - 1) idx = n - 1;
        xr[0 * W + lane] = path[3 * idx];
        xr[1 * W + lane] = path[3 * idx + 1];
        xr[2 * W + lane] = idx >= stop ? 0.0 : (pv ? pv[idx] : a.v_ref);
        xr[3 * W + lane] = path[3 * idx + 2];
        re[lane] = (idx == n - 1);
    }
}

// simulation.py:35-47 + bicycle/main.py:28-41
__device__ __forceinline__ void plant_step(const mpcx_mpc_params &p, double &x, double &y, double &v, double &th,
                                           double a, double delta) {
    delta = fmax(fmin(delta, p.max_steer), -p.max_steer);
    double s, c;
    sincos(th, &s, &c);
    const double xd = __dmul_rn(v, c), yd = __dmul_rn(v, s), td = __dmul_rn(__ddiv_rn(v, p.L), tan(delta));
    x = __dadd_rn(x, __dmul_rn(xd, p.dt));
    y = __dadd_rn(y, __dmul_rn(yd, p.dt));
    th = __dadd_rn(th, __dmul_rn(td, p.dt));
    v = __dadd_rn(v, __dmul_rn(a, p.dt));
    v = fmax(fmin(v, p.max_speed), p.min_speed);
}

struct RollArgs {
    mpcx_mpc_params p;
    int B;
    const double *state, *u_warm;
    double *xbar;
    const int32_t *done;    // retirement (read by the RETIRE instantiation only): the row of an agent with done[b] != 0 is neither computed nor written
};

// Rollout of 64 instances by one wavefront (lane = instance: the reference's operation order, one dependent chain of T x (sincos, tan,
// divide) per instance), results staged in LDS and written as ONE contiguous run: the 64 instances' xbar rows are adjacent in memory
// (64 x 4 x (T+1) doubles).  Until round 3 every lane stored its doubles straight to memory, 8 bytes at a 4 (T+1) x 8-byte lane stride,
// each its own write transaction: 165 MB of write traffic for 45 MB of output.
// (round 4: the staging buffer is dynamic LDS sized for the horizon in use -- 43.5 KB at T = 20 instead of 68 KB for T = 32: this kernel runs
// beside the conflict search on the side stream, and its two workgroups per CU left that kernel's 6.5-KB workgroups 24 KB of a CU's LDS)
// RETIRE: a retired agent's xbar row stays as its last driven step left it (its state and inputs are frozen, so the row would come out
// the same from the step after its arrival on -- but not the same as that last driven step's, which started one state earlier)
template <bool RETIRE>
__global__ __launch_bounds__(64) void rollout_kernel(RollArgs a) {
    extern __shared__ double s_roll[];                   // [64][4 W + 1]; +1: rows of 4 W doubles would sit 8 lanes to a bank group
    const int T = a.p.T, W = T + 1;
    const int RS = 4 * W + 1;
    auto s_x = [&](int lane) -> double * { return s_roll + (size_t)lane * RS; };
    const int b0 = (int)blockIdx.x * 64;
    const int n = a.B - b0 < 64 ? a.B - b0 : 64;
    bool gone = false;
    if constexpr (RETIRE) gone = threadIdx.x < (unsigned)n && a.done[b0 + (int)threadIdx.x] != 0;
    if (threadIdx.x < (unsigned)n && !gone) {
        const int b = b0 + (int)threadIdx.x;
        double x = a.state[4 * b], y = a.state[4 * b + 1], v = a.state[4 * b + 2], th = a.state[4 * b + 3];
        double *xb = s_x(threadIdx.x);
        xb[0] = x; xb[W] = y; xb[2 * W] = v; xb[3 * W] = th;
        const double *oa = a.u_warm ? a.u_warm + (size_t)b * 2 * T : nullptr;
        for (int t = 1; t <= T; t++) {
            const double ai = oa ? oa[t - 1] : 0.0, di = oa ? oa[T + t - 1] : 0.0;   // mpc.py:222-224: zeros when no warm start
            plant_step(a.p, x, y, v, th, ai, di);
            xb[t] = x; xb[W + t] = y; xb[2 * W + t] = v; xb[3 * W + t] = th;
        }
    }
    __syncthreads();
    double *out = a.xbar + (size_t)b0 * 4 * W;
    if constexpr (RETIRE) {
        const unsigned long long gm = __ballot(gone);       // one wavefront per block: bit l = lane l's agent is retired
        for (int i = threadIdx.x; i < n * 4 * W; i += blockDim.x)
            if (!((gm >> (i / (4 * W))) & 1ull)) out[i] = s_x(i / (4 * W))[i % (4 * W)];
    } else
        for (int i = threadIdx.x; i < n * 4 * W; i += blockDim.x) out[i] = s_x(i / (4 * W))[i % (4 * W)];
}

// The two halves of mpc.py:211-239's preparation are independent -- the rollout is a chain of T dependent sincos / tan evaluations per
// instance (44 us), the window selection a scan of the path (31 us) -- and run BESIDE each other: the rollout on the context's side
// stream (fork / join by events, capturable into the closed loop's hipGraph), the window selection on the context's stream.  (Until
// round 3 both were workgroups of one launch; the rollout's 68-KB staging buffer would have been allocated for every workgroup of it.)
// Window workgroups of four wavefronts = four instances: fewer, larger workgroups to dispatch (57 -> 54 us).
constexpr int PREP_WAVES = 4;
template <bool RETIRE>
__global__ __launch_bounds__(64 * PREP_WAVES) void ref_window_kernel(RefArgs ra) {
    const int b = (int)blockIdx.x * PREP_WAVES + (threadIdx.x >> 6);
    if (b < ra.B) ref_window_block<RETIRE>(ra, b);
}

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
        const int it = in ? a.iters[b] : 0;
        const int bad = (in && a.status[b] != MPCX_QP_OPTIMAL) ? 1 : 0;
        int s_it = it, s_bad = bad, s_n = in ? 1 : 0, s_mx = it;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s_it += __shfl_xor(s_it, d, WAVE); s_bad += __shfl_xor(s_bad, d, WAVE); s_n += __shfl_xor(s_n, d, WAVE);
            const int o = __shfl_xor(s_mx, d, WAVE); s_mx = o > s_mx ? o : s_mx;
        }
        if ((threadIdx.x & 63) == 0) {
            // one slot of four counters per wavefront, touched by that wavefront only (steps are ordered by the stream): no atomics --
            // 2048 atomics on four hot words made this 5-us kernel a 22-us one
            unsigned long long *w = a.stats + 4 * (size_t)(b >> 6);
            w[0] += (unsigned long long)s_n; w[1] += (unsigned long long)s_it; w[2] += (unsigned long long)s_bad;
            if ((unsigned long long)s_mx > w[3]) w[3] = (unsigned long long)s_mx;
        }
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
    if (!forked) {
        int32_t rc = mpcx_rollout_fork(ctx, B, state, u_warm, xbar, x.done);
        if (rc != MPCX_OK) return rc;
    }
    // a rollout forked long ago (mpcx_closed_loop_run: at the start of the step) is joined IN FRONT of the window selection: the queue
    // works the barrier off while the conflict search is still running, and nothing stands between the window kernel and the solve;
    // a rollout forked just now runs beside the window selection and is joined behind it
    if (forked && hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "mpc_prepare_batch: cannot join the side stream");
    const dim3 wgrid((B + mpcx::PREP_WAVES - 1) / mpcx::PREP_WAVES), wblock(64 * mpcx::PREP_WAVES);
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
    const size_t roll_lds = 64 * (4 * (size_t)(ctx->mpc.T + 1) + 1) * sizeof(double);
    if (done) hipLaunchKernelGGL(mpcx::rollout_kernel<true>, dim3((B + 63) / 64), dim3(64), roll_lds, ctx->side, ro);
    else hipLaunchKernelGGL(mpcx::rollout_kernel<false>, dim3((B + 63) / 64), dim3(64), roll_lds, ctx->side, ro);
    // a refused launch is the rollout's failure, not that of whichever call checks the error state next (the staging buffer is above
    // 64 KB for T >= 31: gfx950 grants up to 160 KB of LDS per workgroup without hipFuncAttributeMaxDynamicSharedMemorySize)
    const int32_t rc = mpcx_check_launch(ctx, "rollout_kernel");
    if (rc != MPCX_OK) return rc;
    // the join event right behind the rollout: by the time the context's stream waits for it (in front of the solve) the marker has long
    // been processed -- recorded there, the wait paid for the side queue's marker AND its own barrier
    if (hipEventRecord(ctx->ev_join, ctx->side) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "mpc_prepare_batch: cannot record the join event");
    return MPCX_OK;
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
