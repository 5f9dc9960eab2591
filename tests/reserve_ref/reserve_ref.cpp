// Host build of csrc/mpcx_reserve_core.h: the crossing-reservation rule as a plain loop over host arrays.  The GPU's reserve_kernel compiles
// the very same header.  Test infrastructure (tests/test_reserve_cpu.py, tests/test_gpu_reserve.py), also run under the sanitizers as a
// stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_reserve_core.h"

// One step's reservation stage for J junctions of n_per agents, the arguments of the kernel with HOST pointers (done may be null).
// backwards != 0: the junctions are visited from the last to the first (the outcome must not depend on it).  Returns the agents held.
extern "C" int reserve_ref_step(int P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                                int32_t *cut_len, const int32_t *done, const int32_t *path_stop, const int32_t *path_group, int32_t *held,
                                double brake, int n_points, int n_groups, const int32_t *path_exit, const int32_t *conflict, const int32_t *lane,
                                const int32_t *mgr_time, const int32_t *mgr_of, int32_t *grant, int32_t *since, int32_t *clock, int32_t *occupied,
                                int32_t *queued, int n_per, int n_junctions, int n_mgr, int backwards) {
    const mpcx_signals sg = {path_stop, path_group, nullptr, nullptr, nullptr, nullptr, nullptr, held, brake, n_points, 0, n_groups, 0};
    const mpcx_reservation rv = {path_exit, conflict, lane, mgr_time, mgr_of, grant, since, clock, occupied, queued, n_per, n_junctions, n_mgr, 0};
    const mpcx::ReserveArgs a{mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg}, rv};
    int got = 0;
    for (int k = 0; k < n_junctions; k++) got += mpcx::reserve_junction(a, backwards ? n_junctions - 1 - k : k);
    return got;
}

// layout of mpcx_reservation as the header's own compiler has it: sizeof, the offsets of its fourteen fields in order,
// MPCX_RESERVE_PER_MAX; then the sizes of the structs that the reservation travels beside and must not widen: mpcx_closed_loop,
// mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene, mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence, mpcx_signals,
// mpcx_actuation, mpcx_advice, mpcx_intent
extern "C" void reserve_ref_layout(int64_t *out29) {
#define OFF(f) (int64_t)offsetof(mpcx_reservation, f)
    const int64_t v[29] = {(int64_t)sizeof(mpcx_reservation), OFF(path_exit), OFF(conflict), OFF(lane), OFF(mgr_time), OFF(mgr_of), OFF(grant),
                           OFF(since), OFF(clock), OFF(occupied), OFF(queued), OFF(n_per), OFF(n_junctions), OFF(n_mgr), OFF(reserved),
                           MPCX_RESERVE_PER_MAX,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence), (int64_t)sizeof(mpcx_signals),
                           (int64_t)sizeof(mpcx_actuation), (int64_t)sizeof(mpcx_advice), (int64_t)sizeof(mpcx_intent)};
#undef OFF
    for (int i = 0; i < 29; i++) out29[i] = v[i];
}

#ifdef RESERVE_REF_MAIN
// Runs the cases of a file written by tests/test_reserve_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_points, n_groups, n_per, n_junctions, n_mgr, has_done, backwards; double dl, brake; double state (4 P); int32 path_off,
//   path_len, traj_idx, cut_len, done (P each; done only with has_done), path_stop, path_group, path_exit (n_points each), held (P),
//   conflict, lane (n_groups each), mgr_time (2 n_mgr), mgr_of (J), grant, since (P each), clock, occupied, queued (J each)
// out per case: grant, since (P each), clock, occupied, queued (J each), held, cut_len (P each) and the number of agents held, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static void wr(FILE *g, const std::vector<int32_t> &v) { if (!v.empty()) fwrite(v.data(), sizeof(int32_t), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[8];
    while (fread(h, sizeof(int32_t), 8, f) == 8) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], ng = (size_t)h[2], J = (size_t)h[4], nm = (size_t)h[5];
        double d[2];
        if (fread(d, sizeof(double), 2, f) != 2) return 4;
        std::vector<double> state(4 * P);
        if (P && fread(state.data(), sizeof(double), state.size(), f) != state.size()) return 4;
        std::vector<int32_t> off, len, ti, cut, done, stop, grp, ex, held, cf, ln, mt, of, gr, si, ck, oc, qu;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, done, h[6] ? P : 0) || !rd(f, stop, np) || !rd(f, grp, np) ||
            !rd(f, ex, np) || !rd(f, held, P) || !rd(f, cf, ng) || !rd(f, ln, ng) || !rd(f, mt, 2 * nm) || !rd(f, of, J) || !rd(f, gr, P) ||
            !rd(f, si, P) || !rd(f, ck, J) || !rd(f, oc, J) || !rd(f, qu, J))
            return 5;
        const int32_t got = reserve_ref_step((int)P, d[0], state.data(), off.data(), len.data(), ti.data(), cut.data(), h[6] ? done.data() : nullptr,
                                             stop.data(), grp.data(), held.data(), d[1], (int)np, h[2], ex.data(), cf.data(), ln.data(), mt.data(),
                                             of.data(), gr.data(), si.data(), ck.data(), oc.data(), qu.data(), h[3], (int)J, (int)nm, h[7]);
        wr(g, gr); wr(g, si); wr(g, ck); wr(g, oc); wr(g, qu); wr(g, held); wr(g, cut);
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
