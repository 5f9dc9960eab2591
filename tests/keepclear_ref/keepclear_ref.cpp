// Host build of csrc/mpcx_keepclear_core.h: the keep-clear rule as a plain loop over host arrays.  The GPU's keepclear_kernel compiles the
// very same header.  Test infrastructure (tests/test_keepclear_cpu.py, tests/test_gpu_keepclear.py), also run under the sanitizers as a
// stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_keepclear_core.h"

// One step's keep-clear stage for J junctions of n_per agents, the arguments of the kernel with HOST pointers (done may be null).
// backwards != 0: the junctions are visited from the last to the first (the outcome must not depend on it).  Returns the agents boxed.
extern "C" int keepclear_ref_step(int P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                                  int32_t *cut_len, const int32_t *done, const int32_t *path_stop, int32_t *held, double brake, int n_points,
                                  const int32_t *path_move, const int32_t *path_exit, const int32_t *conflict, int32_t *boxed, int32_t *waited,
                                  int32_t *occupied, int32_t *n_boxed, int detect, int n_per, int n_junctions, int n_moves, int backwards) {
    const mpcx_signals sg = {path_stop, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, held, brake, n_points, 0, 0, 0};
    const mpcx_keepclear kc = {path_move, path_exit, conflict, boxed, waited, occupied, n_boxed, detect, n_per, n_junctions, n_moves, n_points, 0};
    const mpcx::KeepClearArgs a{mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg}, kc};
    int got = 0;
    for (int k = 0; k < n_junctions; k++) got += mpcx::keepclear_junction(a, backwards ? n_junctions - 1 - k : k);
    return got;
}

// layout of mpcx_keepclear as the header's own compiler has it: sizeof, the offsets of its thirteen fields in order,
// MPCX_KEEPCLEAR_PER_MAX; then the sizes of the structs that the stage travels beside and must not widen: mpcx_closed_loop,
// mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene, mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence, mpcx_signals,
// mpcx_actuation, mpcx_advice, mpcx_intent, mpcx_reservation, mpcx_following, mpcx_safety, mpcx_sight
extern "C" void keepclear_ref_layout(int64_t *out32) {
#define OFF(f) (int64_t)offsetof(mpcx_keepclear, f)
    const int64_t v[32] = {(int64_t)sizeof(mpcx_keepclear), OFF(path_move), OFF(path_exit), OFF(conflict), OFF(boxed), OFF(waited), OFF(occupied),
                           OFF(n_boxed), OFF(detect), OFF(n_per), OFF(n_junctions), OFF(n_moves), OFF(n_points), OFF(reserved),
                           MPCX_KEEPCLEAR_PER_MAX,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence), (int64_t)sizeof(mpcx_signals),
                           (int64_t)sizeof(mpcx_actuation), (int64_t)sizeof(mpcx_advice), (int64_t)sizeof(mpcx_intent),
                           (int64_t)sizeof(mpcx_reservation), (int64_t)sizeof(mpcx_following), (int64_t)sizeof(mpcx_safety),
                           (int64_t)sizeof(mpcx_sight)};
#undef OFF
    for (int i = 0; i < 32; i++) out32[i] = v[i];
}

#ifdef KEEPCLEAR_REF_MAIN
// Runs the cases of a file written by tests/test_keepclear_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_points, n_moves, n_per, n_junctions, detect, has_done, backwards; double dl, brake; double state (4 P); int32 path_off,
//   path_len, traj_idx, cut_len, done (P each; done only with has_done), path_stop, path_move, path_exit (n_points each), held (P),
//   conflict (n_moves), boxed, waited (P each), occupied, n_boxed (J each)
// out per case: cut_len, boxed, waited (P each), occupied, n_boxed (J each) and the number of agents boxed, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static void wr(FILE *g, const std::vector<int32_t> &v) { if (!v.empty()) fwrite(v.data(), sizeof(int32_t), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[8];
    while (fread(h, sizeof(int32_t), 8, f) == 8) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], nm = (size_t)h[2], J = (size_t)h[4];
        double d[2];
        if (fread(d, sizeof(double), 2, f) != 2) return 4;
        std::vector<double> state(4 * P);
        if (P && fread(state.data(), sizeof(double), state.size(), f) != state.size()) return 4;
        std::vector<int32_t> off, len, ti, cut, done, stop, mv, ex, held, cf, bx, wt, oc, nb;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, done, h[6] ? P : 0) || !rd(f, stop, np) || !rd(f, mv, np) ||
            !rd(f, ex, np) || !rd(f, held, P) || !rd(f, cf, nm) || !rd(f, bx, P) || !rd(f, wt, P) || !rd(f, oc, J) || !rd(f, nb, J))
            return 5;
        const int32_t got = keepclear_ref_step((int)P, d[0], state.data(), off.data(), len.data(), ti.data(), cut.data(), h[6] ? done.data() : nullptr,
                                               stop.data(), held.data(), d[1], (int)np, mv.data(), ex.data(), cf.data(), bx.data(), wt.data(),
                                               oc.data(), nb.data(), h[5], h[3], (int)J, (int)nm, h[7]);
        wr(g, cut); wr(g, bx); wr(g, wt); wr(g, oc); wr(g, nb);
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
