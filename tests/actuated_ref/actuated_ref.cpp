// Host build of csrc/mpcx_actuated_core.h: the vehicle-actuated signal rule as a plain loop over host arrays.  The GPU's
// actuated_signal_kernel compiles the very same header.  Test infrastructure (tests/test_actuated_cpu.py, tests/test_gpu_actuated.py), also
// run under the sanitizers as a stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_actuated_core.h"

// One step's actuated signal stage for J junctions of n_per agents, the arguments of the kernel with HOST pointers (done may be null).
// backwards != 0: the junctions are visited from the last to the first (the outcome must not depend on it).  Returns the agents held.
extern "C" int actuated_ref_step(int P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                                 int32_t *cut_len, const int32_t *done, const int32_t *path_stop, const int32_t *path_group, int32_t *held,
                                 double brake, int n_points, int n_groups, const int32_t *phase_groups, const int32_t *phase_time,
                                 const int32_t *ctrl_time, const int32_t *ctrl_of, int32_t *jstate, int32_t *lights, int32_t *calls, int n_per,
                                 int n_junctions, int n_phases, int n_ctrl, int backwards) {
    const mpcx_signals sg = {path_stop, path_group, nullptr, nullptr, nullptr, nullptr, nullptr, held, brake, n_points, 0, n_groups, 0};
    const mpcx_actuation ac = {phase_groups, phase_time, ctrl_time, ctrl_of, jstate, lights, calls, n_per, n_junctions, n_phases, n_ctrl, 0};
    const mpcx::ActuatedArgs a{mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg}, ac};
    int got = 0;
    for (int k = 0; k < n_junctions; k++) got += mpcx::actuated_junction(a, backwards ? n_junctions - 1 - k : k);
    return got;
}

// layout of mpcx_actuation as the header's own compiler has it: sizeof, the offsets of its twelve fields in order,
// MPCX_ACTUATION_PHASES_MAX; then the sizes of the structs that actuation travels beside and must not widen: mpcx_closed_loop,
// mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene, mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence, mpcx_signals
extern "C" void actuated_ref_layout(int64_t *out24) {
#define OFF(f) (int64_t)offsetof(mpcx_actuation, f)
    const int64_t v[24] = {(int64_t)sizeof(mpcx_actuation), OFF(phase_groups), OFF(phase_time), OFF(ctrl_time), OFF(ctrl_of), OFF(jstate),
                           OFF(lights), OFF(calls), OFF(n_per), OFF(n_junctions), OFF(n_phases), OFF(n_ctrl), OFF(reserved),
                           MPCX_ACTUATION_PHASES_MAX,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence), (int64_t)sizeof(mpcx_signals)};
#undef OFF
    for (int i = 0; i < 24; i++) out24[i] = v[i];
}

#ifdef ACTUATED_REF_MAIN
// Runs the cases of a file written by tests/test_actuated_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_points, n_groups, n_per, n_junctions, n_phases, n_ctrl, has_done, backwards; double dl, brake; double state (4 P); int32
//   path_off, path_len, traj_idx, cut_len, done (P each; done only with has_done), path_stop, path_group (n_points each), held (P),
//   phase_groups (n_ctrl n_phases), phase_time (3 n_ctrl n_phases), ctrl_time (3 n_ctrl), ctrl_of (J), jstate (4 J), lights, calls (J each)
// out per case: jstate (4 J), lights, calls (J each), held, cut_len (P each) and the number of agents held, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static void wr(FILE *g, const std::vector<int32_t> &v) { if (!v.empty()) fwrite(v.data(), sizeof(int32_t), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[9];
    while (fread(h, sizeof(int32_t), 9, f) == 9) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], J = (size_t)h[4], nph = (size_t)h[5], nc = (size_t)h[6];
        double d[2];
        if (fread(d, sizeof(double), 2, f) != 2) return 4;
        std::vector<double> state(4 * P);
        if (P && fread(state.data(), sizeof(double), state.size(), f) != state.size()) return 4;
        std::vector<int32_t> off, len, ti, cut, done, stop, grp, held, pg, pt, ct, of, js, li, ca;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, done, h[7] ? P : 0) || !rd(f, stop, np) || !rd(f, grp, np) ||
            !rd(f, held, P) || !rd(f, pg, nc * nph) || !rd(f, pt, 3 * nc * nph) || !rd(f, ct, 3 * nc) || !rd(f, of, J) || !rd(f, js, 4 * J) ||
            !rd(f, li, J) || !rd(f, ca, J))
            return 5;
        const int32_t got = actuated_ref_step((int)P, d[0], state.data(), off.data(), len.data(), ti.data(), cut.data(), h[7] ? done.data() : nullptr,
                                              stop.data(), grp.data(), held.data(), d[1], (int)np, h[2], pg.data(), pt.data(), ct.data(), of.data(),
                                              js.data(), li.data(), ca.data(), h[3], (int)J, (int)nph, (int)nc, h[8]);
        wr(g, js); wr(g, li); wr(g, ca); wr(g, held); wr(g, cut);
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
