// Host build of csrc/mpcx_signal_core.h: the traffic-signal rule as a plain loop over host arrays.  The GPU's signal_kernel compiles the
// very same header.  Test infrastructure (tests/test_signal_cpu.py, tests/test_gpu_signal.py), also run under the sanitizers as a
// stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_signal_core.h"

// One step's signal stage for P agents, the arguments of the kernel with HOST pointers (done may be null).  backwards != 0: the lanes are
// visited from the last to the first (the outcome must not depend on it).  Returns the number of agents held.
extern "C" int signal_ref_step(int P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                               int32_t *cut_len, const int32_t *done, const int32_t *path_stop, const int32_t *path_group,
                               const int32_t *plan_cycle, const int32_t *plan_amber, const int32_t *plan_green, const int32_t *plan_of,
                               int32_t *tick, int32_t *held, double brake, int n_points, int n_plans, int n_groups, int backwards) {
    const mpcx_signals sg = {path_stop, path_group, plan_cycle, plan_amber, plan_green, plan_of, tick, held, brake, n_points, n_plans, n_groups, 0};
    const mpcx::SignalArgs a{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg};
    int got = 0;
    for (int k = 0; k < P; k++) got += mpcx::signal_agent(a, backwards ? P - 1 - k : k) != 0 ? 1 : 0;
    return got;
}

// layout of mpcx_signals as the header's own compiler has it: sizeof, the offsets of its thirteen fields in order, MPCX_SIGNAL_GROUPS_MAX;
// then the sizes of the structs that signals travel beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log,
// mpcx_retire, mpcx_scene, mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence
extern "C" void signal_ref_layout(int64_t *out24) {
#define OFF(f) (int64_t)offsetof(mpcx_signals, f)
    const int64_t v[24] = {(int64_t)sizeof(mpcx_signals), OFF(path_stop), OFF(path_group), OFF(plan_cycle), OFF(plan_amber), OFF(plan_green),
                           OFF(plan_of), OFF(tick), OFF(held), OFF(brake), OFF(n_points), OFF(n_plans), OFF(n_groups), OFF(reserved),
                           MPCX_SIGNAL_GROUPS_MAX,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence)};
#undef OFF
    for (int i = 0; i < 24; i++) out24[i] = v[i];
}

#ifdef SIGNAL_REF_MAIN
// Runs the cases of a file written by tests/test_signal_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_points, n_plans, n_groups, has_done, backwards; double dl, brake; double state (4 P); int32 path_off, path_len, traj_idx,
//   cut_len, done (P each; done only with has_done), path_stop, path_group (n_points each), plan_cycle, plan_amber (n_plans each),
//   plan_green (2 n_plans n_groups), plan_of, tick, held (P each)
// out per case: cut_len, tick, held (P each) and the number of agents held, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[6];
    while (fread(h, sizeof(int32_t), 6, f) == 6) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], npl = (size_t)h[2], ng = (size_t)h[3];
        double d[2];
        if (fread(d, sizeof(double), 2, f) != 2) return 4;
        std::vector<double> state(4 * P);
        if (P && fread(state.data(), sizeof(double), state.size(), f) != state.size()) return 4;
        std::vector<int32_t> off, len, ti, cut, done, stop, grp, cyc, amb, grn, of, tick, held;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, done, h[4] ? P : 0) || !rd(f, stop, np) || !rd(f, grp, np) ||
            !rd(f, cyc, npl) || !rd(f, amb, npl) || !rd(f, grn, 2 * npl * ng) || !rd(f, of, P) || !rd(f, tick, P) || !rd(f, held, P))
            return 5;
        const int32_t got = signal_ref_step((int)P, d[0], state.data(), off.data(), len.data(), ti.data(), cut.data(), h[4] ? done.data() : nullptr,
                                            stop.data(), grp.data(), cyc.data(), amb.data(), grn.data(), of.data(), tick.data(), held.data(), d[1],
                                            (int)np, (int)npl, (int)ng, h[5]);
        if (P) {
            fwrite(cut.data(), sizeof(int32_t), P, g);
            fwrite(tick.data(), sizeof(int32_t), P, g);
            fwrite(held.data(), sizeof(int32_t), P, g);
        }
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
