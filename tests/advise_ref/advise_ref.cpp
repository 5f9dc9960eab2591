// Host build of csrc/mpcx_advise_core.h: the signal-aware approach-speed rule as a plain loop over host arrays.  The GPU's advise_kernel
// compiles the very same header.  Test infrastructure (tests/test_advise_cpu.py, tests/test_gpu_advise.py), also run under the sanitizers
// as a stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_advise_core.h"

// One step's advice stage for P agents with windows of W = T + 1 points, the arguments of the kernel with HOST pointers (done may be
// null).  backwards != 0: the lanes are visited from the last to the first (the outcome must not depend on it).  Writes advised (P) and
// row 2 of every advised agent's xref (P x 4 x W); returns the number of agents advised.
extern "C" int advise_ref_step(int P, int W, double dl, double dt, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                               const int32_t *cut_len, const int32_t *done, const int32_t *path_stop, const int32_t *path_group,
                               const int32_t *plan_cycle, const int32_t *plan_amber, const int32_t *plan_green, const int32_t *plan_of,
                               const int32_t *tick, int n_points, int n_plans, int n_groups, double *advised, double v_cruise, double v_min,
                               double reach, int lead, double *xref, int backwards) {
    mpcx::AdviseArgs a;
    a.P = P; a.W = W; a.dl = dl; a.dt = dt;
    a.path_off = path_off; a.path_len = path_len; a.traj_idx = traj_idx; a.cut_len = cut_len; a.done = done; a.xref = xref;
    a.sg = {path_stop, path_group, plan_cycle, plan_amber, plan_green, plan_of, const_cast<int32_t *>(tick), nullptr, 1.0, n_points, n_plans, n_groups, 0};
    a.ad = {advised, v_cruise, v_min, reach, lead, P};
    int got = 0;
    for (int k = 0; k < P; k++) got += mpcx::advise_agent(a, backwards ? P - 1 - k : k) > 0.0 ? 1 : 0;
    return got;
}

// layout of mpcx_advice as the header's own compiler has it: sizeof, the offsets of its six fields in order; then the sizes of the structs
// that advice travels beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene,
// mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence, mpcx_signals, mpcx_actuation
extern "C" void advise_ref_layout(int64_t *out18) {
#define OFF(f) (int64_t)offsetof(mpcx_advice, f)
    const int64_t v[18] = {(int64_t)sizeof(mpcx_advice), OFF(advised), OFF(v_cruise), OFF(v_min), OFF(reach), OFF(lead), OFF(n_rows),
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence), (int64_t)sizeof(mpcx_signals),
                           (int64_t)sizeof(mpcx_actuation)};
#undef OFF
    for (int i = 0; i < 18; i++) out18[i] = v[i];
}

#ifdef ADVISE_REF_MAIN
// Runs the cases of a file written by tests/test_advise_cpu.py and writes every case's words back.  Per case:
//   int32 P, W, n_points, n_plans, n_groups, has_done, backwards, lead; double dl, dt, v_cruise, v_min, reach; int32 path_off, path_len,
//   traj_idx, cut_len, done (P each; done only with has_done), path_stop, path_group (n_points each), plan_cycle, plan_amber (n_plans each),
//   plan_green (2 n_plans n_groups), plan_of, tick (P each); double xref (4 P W)
// out per case: advised (P doubles), xref (4 P W doubles) and the number of agents advised, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[8];
    while (fread(h, sizeof(int32_t), 8, f) == 8) {
        const size_t P = (size_t)h[0], W = (size_t)h[1], np = (size_t)h[2], npl = (size_t)h[3], ng = (size_t)h[4];
        double d[5];
        if (fread(d, sizeof(double), 5, f) != 5) return 4;
        std::vector<int32_t> off, len, ti, cut, done, stop, grp, cyc, amb, grn, of, tick;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, done, h[5] ? P : 0) || !rd(f, stop, np) || !rd(f, grp, np) ||
            !rd(f, cyc, npl) || !rd(f, amb, npl) || !rd(f, grn, 2 * npl * ng) || !rd(f, of, P) || !rd(f, tick, P))
            return 5;
        std::vector<double> xref(4 * P * W), advised(P);
        if (!xref.empty() && fread(xref.data(), sizeof(double), xref.size(), f) != xref.size()) return 6;
        const int32_t got = advise_ref_step((int)P, (int)W, d[0], d[1], off.data(), len.data(), ti.data(), cut.data(), h[5] ? done.data() : nullptr,
                                            stop.data(), grp.data(), cyc.data(), amb.data(), grn.data(), of.data(), tick.data(), (int)np, (int)npl,
                                            (int)ng, advised.data(), d[2], d[3], d[4], h[7], xref.data(), h[6]);
        if (P) {
            fwrite(advised.data(), sizeof(double), P, g);
            fwrite(xref.data(), sizeof(double), xref.size(), g);
        }
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
