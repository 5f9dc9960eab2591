// Host build of csrc/mpcx_priority_core.h: the priority rule as a plain loop over host arrays.  The GPU's priority_kernel compiles the very
// same header.  Test infrastructure (tests/test_priority_cpu.py, tests/test_gpu_priority.py), also run under the sanitizers as a
// stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mpcx_priority_core.h"

// One step's priority stage for J junctions of n_per agents, the arguments of the kernel with HOST pointers (done may be null).
// backwards != 0: the junctions are visited from the last to the first (the outcome must not depend on it).  Returns the agents yielding.
extern "C" int priority_ref_step(int P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                                 int32_t *cut_len, const int32_t *done, const int32_t *path_stop, const int32_t *path_move, const int32_t *path_exit,
                                 const int32_t *conflict, const int32_t *rank, const double *gap, int32_t *waited, int32_t *yielding,
                                 int32_t *blocker, double *lag, int32_t *occupied, int32_t *n_yielding, double v_floor, double brake, int detect,
                                 int n_per, int n_junctions, int n_moves, int n_points, int backwards) {
    mpcx_signals sg;
    memset(&sg, 0, sizeof sg);
    sg.path_stop = path_stop;
    const mpcx_priority pr = {path_stop, path_move, path_exit, conflict, rank, gap, waited, yielding, blocker, lag, occupied, n_yielding,
                              v_floor, brake, detect, n_per, n_junctions, n_moves, n_points, 0};
    const mpcx::PriorityArgs a{mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg}, pr};
    int got = 0;
    for (int k = 0; k < n_junctions; k++) got += mpcx::priority_junction(a, backwards ? n_junctions - 1 - k : k);
    return got;
}

// layout of mpcx_priority as the header's own compiler has it: sizeof, the offsets of its twenty fields in order, MPCX_PRIORITY_PER_MAX;
// then the sizes of the structs that the stage travels beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log,
// mpcx_retire, mpcx_scene, mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence, mpcx_signals, mpcx_actuation, mpcx_advice, mpcx_intent,
// mpcx_reservation, mpcx_following, mpcx_safety, mpcx_sight, mpcx_keepclear
extern "C" void priority_ref_layout(int64_t *out40) {
#define OFF(f) (int64_t)offsetof(mpcx_priority, f)
    const int64_t v[40] = {(int64_t)sizeof(mpcx_priority), OFF(path_stop), OFF(path_move), OFF(path_exit), OFF(conflict), OFF(rank), OFF(gap),
                           OFF(waited), OFF(yielding), OFF(blocker), OFF(lag), OFF(occupied), OFF(n_yielding), OFF(v_floor), OFF(brake),
                           OFF(detect), OFF(n_per), OFF(n_junctions), OFF(n_moves), OFF(n_points), OFF(reserved), MPCX_PRIORITY_PER_MAX,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence), (int64_t)sizeof(mpcx_signals),
                           (int64_t)sizeof(mpcx_actuation), (int64_t)sizeof(mpcx_advice), (int64_t)sizeof(mpcx_intent),
                           (int64_t)sizeof(mpcx_reservation), (int64_t)sizeof(mpcx_following), (int64_t)sizeof(mpcx_safety),
                           (int64_t)sizeof(mpcx_sight), (int64_t)sizeof(mpcx_keepclear)};
#undef OFF
    for (int i = 0; i < 40; i++) out40[i] = v[i];
}

#ifdef PRIORITY_REF_MAIN
// Runs the cases of a file written by tests/test_priority_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_points, n_moves, n_per, n_junctions, detect, has_done, backwards; double dl, v_floor, brake; double state (4 P); int32
//   path_off, path_len, traj_idx, cut_len, done (P each; done only with has_done), path_stop, path_move, path_exit (n_points each),
//   conflict, rank (n_moves each); double gap (n_moves); int32 waited, yielding, blocker (P each); double lag (P); int32 occupied,
//   n_yielding (J each)
// out per case: cut_len, waited, yielding, blocker (P each, int32), lag (P doubles), occupied, n_yielding (J each) and the number of agents
// yielding, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static bool rdd(FILE *f, std::vector<double> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(double), n, f) == n; }
static void wr(FILE *g, const std::vector<int32_t> &v) { if (!v.empty()) fwrite(v.data(), sizeof(int32_t), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[8];
    while (fread(h, sizeof(int32_t), 8, f) == 8) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], nm = (size_t)h[2], J = (size_t)h[4];
        double d[3];
        if (fread(d, sizeof(double), 3, f) != 3) return 4;
        std::vector<double> state, gap, lag;
        std::vector<int32_t> off, len, ti, cut, done, stop, mv, ex, cf, rk, wt, yl, bl, oc, ny;
        if (!rdd(f, state, 4 * P) || !rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, done, h[6] ? P : 0) ||
            !rd(f, stop, np) || !rd(f, mv, np) || !rd(f, ex, np) || !rd(f, cf, nm) || !rd(f, rk, nm) || !rdd(f, gap, nm) || !rd(f, wt, P) ||
            !rd(f, yl, P) || !rd(f, bl, P) || !rdd(f, lag, P) || !rd(f, oc, J) || !rd(f, ny, J))
            return 5;
        const int32_t got = priority_ref_step((int)P, d[0], state.data(), off.data(), len.data(), ti.data(), cut.data(), h[6] ? done.data() : nullptr,
                                              stop.data(), mv.data(), ex.data(), cf.data(), rk.data(), gap.data(), wt.data(), yl.data(), bl.data(),
                                              lag.data(), oc.data(), ny.data(), d[1], d[2], h[5], h[3], (int)J, (int)nm, (int)np, h[7]);
        wr(g, cut); wr(g, wt); wr(g, yl); wr(g, bl);
        if (!lag.empty()) fwrite(lag.data(), sizeof(double), lag.size(), g);
        wr(g, oc); wr(g, ny);
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
