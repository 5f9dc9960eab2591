// mpcx_qp_quad.hip -- device build of the stage-structured QP solver (mpcx_qp_stage.h): EIGHT lanes per problem, eight
// problems per wavefront.  Lane q of a group owns stages q*SPL ..
// q*SPL+SPL-1; the Riccati / costate / rollout sweeps hand their carry to the neighbour lane with row_shl:1 / row_shr:1 DPP
// moves (full rate, no LDS), group reductions are three DPP butterflies, slacks / multipliers / the state block of the gains
// live in LDS as [row][lane] (conflict-free, 36 KB per workgroup at SPL = 3 = four workgroups per CU), everything else in
// registers.  Wavefronts are persistent: groups draw problems from a global ticket (QueueSrc).
#include "mpcx_common.h"
#include "mpcx_qp_stage.h"

namespace mpcx {

typedef __attribute__((address_space(3))) double lds_double;

// group geometry: 8 lanes (row shifts + half-row mirror) inside one DPP row of 16 lanes
template <int LQ_, int SPL_, bool JERK_ = false>
struct GroupCx {
    static constexpr int LQ = LQ_, SPL = SPL_;
    static constexpr bool JERK = JERK_;       // the five-state problem of lib/mpc_jerk.py (mpcx_mpc_params.model)
    static_assert(LQ == 8, "groups of 8 lanes");
    // plain copies of the predictor's and of the corrector's row pass (mpcx_qp_stage.h).  Every instantiation takes the same two: each has
    // less scratch with them than without (DESIGN 4.1 has the list, the counts and the timings).  The residual pass gets none: with all
    // three copies the five-state kernel at SPL = 4 gave wrong solutions (cause not found; each pair of copies is right).  The multiplier
    // step and the update get none: with theirs the scratch of every SPL = 3 and 4 instantiation goes up and the launch gets slower.
    static constexpr int PLAIN_PASSES = mpcx_stage::PLAIN_C | mpcx_stage::PLAIN_D;
    int q, lane;
    lds_double *sh;                       // s [SPL*8][64], lam [SPL*8][64], gains [SPL*8][64], spare [2*SPL][64]
    // row_shl:1 / row_shr:1 = value of lane q+1 / q-1.
    // The value arriving at a group's edge lane comes from the neighbouring group and is never used.
    __device__ __forceinline__ double nxt(double v) const { return dpp_mov<0x101>(v, v); }
    __device__ __forceinline__ double prv(double v) const { return dpp_mov<0x111>(v, v); }
    // butterflies: quad_perm [1,0,3,2] (xor 1), [2,3,0,1] (xor 2), row_half_mirror (lane i <-> 7-i of each half row)
    __device__ __forceinline__ double gsum(double v) const {
        v += dpp_mov<0xB1>(v, v); v += dpp_mov<0x4E>(v, v);
        v += dpp_mov<0x141>(v, v);
        return v;
    }
    __device__ __forceinline__ double gmax(double v) const {
        v = fmax(v, dpp_mov<0xB1>(v, v)); v = fmax(v, dpp_mov<0x4E>(v, v));
        v = fmax(v, dpp_mov<0x141>(v, v));
        return v;
    }
    __device__ __forceinline__ double gmin(double v) const {
        v = fmin(v, dpp_mov<0xB1>(v, v)); v = fmin(v, dpp_mov<0x4E>(v, v));
        v = fmin(v, dpp_mov<0x141>(v, v));
        return v;
    }
    __device__ __forceinline__ bool gany(bool b) const {
        const unsigned long long m = __ballot(b);
        return ((m >> (lane & ~(LQ - 1))) & ((1ull << LQ) - 1ull)) != 0ull;
    }
    __device__ __forceinline__ bool any(bool b) const { return __ballot(b) != 0ull; }
    __device__ __forceinline__ int count(bool b) const { return __popcll(__ballot(b)); }       // lanes, not groups
    __device__ __forceinline__ double rcp(double v) const { return frcp(v); }
    __device__ __forceinline__ double rcp_fast(double v) const { return frcp1(v); }     // seed + one Newton step
    // ratio tests only: the hardware seed; the 0.001 margin of the step fraction is four orders of magnitude wider than its error
    __device__ __forceinline__ double rcp_seed(double v) const { return __builtin_amdgcn_rcp(v); }
    // phase boundary: LDS values are re-read afterwards instead of being carried in registers across the phase
    __device__ __forceinline__ void fence() const { asm volatile("" ::: "memory"); }
    // phase-boundary marker of solve_queue: empty in every build.  The calls stay because the compiled stage kernel changes without them
    // (registers, spills and scratch of the SPL = 3 and 4 instances move) although they emit no instruction themselves.
    __device__ __forceinline__ void stamp(int) const {}
    __device__ __forceinline__ double ld_s(int k) const { return sh[(0 * SPL * 8 + k) * 64 + lane]; }
    __device__ __forceinline__ double ld_l(int k) const { return sh[(1 * SPL * 8 + k) * 64 + lane]; }
    __device__ __forceinline__ double ld_k(int k) const { return sh[(2 * SPL * 8 + k) * 64 + lane]; }
    __device__ __forceinline__ void st_s(int k, double v) { sh[(0 * SPL * 8 + k) * 64 + lane] = v; }
    __device__ __forceinline__ void st_l(int k, double v) { sh[(1 * SPL * 8 + k) * 64 + lane] = v; }
    __device__ __forceinline__ void st_k(int k, double v) { sh[(2 * SPL * 8 + k) * 64 + lane] = v; }
    __device__ __forceinline__ double ld_w(int k) const { return sh[(3 * SPL * 8 + k) * 64 + lane]; }     // per-problem constants (2 * SPL per lane)
    __device__ __forceinline__ void st_w(int k, double v) { sh[(3 * SPL * 8 + k) * 64 + lane] = v; }
};

// work queue: group leaders draw problem indices from a global ticket until the batch is exhausted; idle groups are refilled
// once REFILL_GROUPS of them are waiting (or nobody is running any more)
constexpr int REFILL_GROUPS = 2;
template <int LQ, int SPL, bool TUNED, bool JERK>
struct QueueSrc {
    const QpArgs &a;
    // The compiler loads every field of the by-value argument once, at the kernel's entry, and keeps it in scalar registers.  A round
    // reads few of them (the rows' bounds, dt, tol, T); the thirteen base pointers and the queue's words are read only by the draw, the
    // set-up and the hand-in, yet were held across every round, spilled to and reloaded from VGPR lanes all over the row passes and
    // sweeps.  With LATE_ARGS, at() and fetch() read them through late(): the kernel-argument segment again (QpArgs is the
    // kernel's only argument, so it lies at offset 0), behind an empty asm that hides from the compiler that the pointer is the same every
    // time.  Its loads stay where they are written, scalar loads at the refill.
    // On for the four-state kernel without tuning rows at SPL = 3 only: that is the instantiation whose time was measured with it (six
    // alternating pairs against the parent).  The other eleven read `a` as before and compile to the code they had; their static
    // counts with late reads are in DESIGN 4.1 (ten of them better, <8,4,false,false> with more scratch), none of them timed.
    static constexpr bool LATE_ARGS = SPL == 3 && !TUNED && !JERK;
    typedef const __attribute__((address_space(4))) QpArgs *LateArgs;
    __device__ __forceinline__ auto late() const {
        if constexpr (LATE_ARGS) {
            LateArgs pa = (LateArgs)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(pa));
            return pa;
        } else return &a;
    }
    __device__ __forceinline__ mpcx_mpc_params params() const { return a.p; }
    __device__ __forceinline__ bool plain_rounds() const { return a.plain_rounds != 0; }     // mpcx_qp_set_plain_rounds
    __device__ __forceinline__ mpcx_stage::Problem at(int b) const {
        const auto l = late();
        const int T = a.p.T, W = T + 1;
        return mpcx_stage::Problem{l->x0 + (size_t)b * 4, l->xref + (size_t)b * 4 * W, l->xbar + (size_t)b * 4 * W,
                                   l->has_warm ? l->u_warm + (size_t)b * 2 * T : nullptr, l->re + (size_t)b * W,
                                   l->x_out + (size_t)b * 4 * W, l->u_out + (size_t)b * 2 * T, l->kkt + (size_t)b * 4,
                                   l->status + b, l->iters + b};
    }
    // every round either advances some group's iteration counter or consumes a ticket
    __device__ __forceinline__ int refill_min() const { return REFILL_GROUPS * LQ; }   // in lanes
    __device__ __forceinline__ long max_rounds() const { return ((long)a.B + 2) * (long)(a.p.max_iter + 6) * (MPCX_POLISH_TRIES + 1); }
    template <class Cx>
    __device__ __forceinline__ bool fetch(Cx &cx, mpcx_mpc_params &P, int &pbi) const {
        const auto l = late();
        int t = 0;
        if (cx.q == 0) t = atomicAdd(l->ticket, 1);
        t = (int)cx.gsum((double)t);                  // the other lanes contribute 0: everybody gets the leader's ticket
        const bool have = t < (l->has_queue_len ? *l->queue_len : l->B);
        const int b = have ? (l->has_order ? l->order[t] : t) : 0;
        pbi = b;
        if (TUNED) {
            const mpcx_qp_tuning &tu = l->tune[b];
            P.w_perp = tu.w_perp; P.w_para = tu.w_para;
            P.R[0] = tu.R[0]; P.R[1] = tu.R[1]; P.Rd[0] = tu.Rd[0]; P.Rd[1] = tu.Rd[1];
            P.Q_v_yaw[0] = tu.Q_v_yaw[0]; P.Q_v_yaw[1] = tu.Q_v_yaw[1];
            P.Qf[0] = tu.Qf[0]; P.Qf[1] = tu.Qf[1]; P.Qf[2] = tu.Qf[2]; P.Qf[3] = tu.Qf[3];
            P.max_accel = tu.max_accel; P.max_decel = tu.max_decel; P.max_dsteer = tu.max_dsteer;
        }
        return have;
    }
};

template <int LQ, int SPL, bool TUNED, bool JERK>
__global__ __launch_bounds__(64, 1) void qp_quad_kernel(QpArgs a) {
    // the second-chance launch behind the condensed solver finds its list empty on (almost) every step: leave before the set-up of
    // eight empty lane groups and the first residual pass (that was 16 us per step at 4096 problems per GPU, the 8-GPU regime)
    if (a.has_queue_len && *a.queue_len == 0) return;
    __shared__ double sh[(3 * SPL * 8 + 2 * SPL) * 64];
    const int lane = threadIdx.x;
    GroupCx<LQ, SPL, JERK> cx{lane & (LQ - 1), lane, (lds_double *)sh};
    QueueSrc<LQ, SPL, TUNED, JERK> src{a};
    mpcx_stage::solve_queue(cx, src);
}

int qp_stage_grid(int B, int n_cu) {
    const int need = (B + 7) / 8;       // eight lane groups per wavefront
    const int resident = n_cu * 4;      // one wavefront per SIMD
    return need < resident ? need : resident;
}

template <int LQ, int SPL, bool JERK>
void launch_qp_group(const QpArgs &a, hipStream_t st, int n_cu) {
    static_assert(LQ == 8, "qp_stage_grid counts eight lane groups per wavefront");
    const int grid = qp_stage_grid(a.B, n_cu);
    if (a.has_tune) hipLaunchKernelGGL((qp_quad_kernel<LQ, SPL, true, JERK>), dim3(grid), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((qp_quad_kernel<LQ, SPL, false, JERK>), dim3(grid), dim3(64), 0, st, a);
}

void launch_qp_stage(const QpArgs &a, hipStream_t st, int n_cu) {
    const int T = a.p.T;
    if (a.p.model == MPCX_MODEL_JERK5) {
        if (T <= 16) launch_qp_group<8, 2, true>(a, st, n_cu);
        else if (T <= 24) launch_qp_group<8, 3, true>(a, st, n_cu);
        else launch_qp_group<8, 4, true>(a, st, n_cu);
        return;
    }
    if (T <= 16) launch_qp_group<8, 2, false>(a, st, n_cu);
    else if (T <= 24) launch_qp_group<8, 3, false>(a, st, n_cu);
    else launch_qp_group<8, 4, false>(a, st, n_cu);
}

}  // namespace mpcx
