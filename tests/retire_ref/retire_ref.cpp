// Host build of csrc/mpcx_retire_core.h (retirement at the goal for one agent and step; the GPU's retire_kernel compiles the very same
// header): test infrastructure that feeds it the reference's recorded runs and lets the sanitizers see it.  Never loaded by the product path.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_retire_core.h"

// one step's retirement test for P agents, the arguments of retire_kernel with HOST pointers; returns the number of agents that arrived
extern "C" int retire_ref_step(int P, const double *state, double *applied, const double *path_xyyaw, const int32_t *path_off,
                               const int32_t *path_len, const int32_t *target_ind, const int32_t *goal_len, const mpcx_retire *r) {
    mpcx::RetireArgs a{P, state, path_xyyaw, applied, path_off, path_len, target_ind, goal_len, *r};
    int n = 0;
    for (int q = 0; q < P; q++) n += mpcx::retire_agent(a, q) ? 1 : 0;
    return n;
}

// layout of mpcx_retire as the header's own compiler has it: sizeof, then the offsets of its fields in order; then the sizes of
// mpcx_closed_loop, mpcx_closed_loop_opts and mpcx_run_log, none of which retirement widens
extern "C" void retire_ref_layout(int64_t *out8) {
    const size_t v[8] = {sizeof(mpcx_retire), offsetof(mpcx_retire, done), offsetof(mpcx_retire, steps_driven), offsetof(mpcx_retire, goal_dis),
                         offsetof(mpcx_retire, stop_speed), sizeof(mpcx_closed_loop), sizeof(mpcx_closed_loop_opts), sizeof(mpcx_run_log)};
    for (int i = 0; i < 8; i++) out8[i] = (int64_t)v[i];
}

// A self-contained case that walks every branch of the rule on seeded pseudo-random data: agents that arrive (at different steps), one that
// is retired from the start, one that comes close but too fast, one whose target index is far from the path end, one with an empty path.
// out: per step and agent (done, steps_driven, applied[0], applied[1]) as doubles (n_out = retire_ref_selfcase_size()).
enum { SC_P = 6, SC_STEPS = 8, SC_NPTS = 30 };
extern "C" int retire_ref_selfcase_size(void) { return SC_STEPS * SC_P * 4; }
extern "C" void retire_ref_selfcase(double *out) {
    uint64_t seed = 4711;
    auto rnd = [&seed]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
    std::vector<double> path(3 * SC_NPTS), state(4 * SC_P), applied(2 * SC_P);
    for (int i = 0; i < SC_NPTS; i++) { path[3 * i] = 0.5 * i; path[3 * i + 1] = 0.1 * i; path[3 * i + 2] = 0.2; }
    const int32_t path_off[SC_P] = {0, 0, 10, 10, 0, 29}, path_len[SC_P] = {10, 10, 20, 20, 30, 0};
    std::vector<int32_t> target(SC_P), goal_len(SC_P), done(SC_P, 0), driven(SC_P, 0);
    done[1] = 1;
    mpcx_retire r = {done.data(), driven.data(), 1.5, 0.1389};
    size_t o = 0;
    for (int s = 0; s < SC_STEPS; s++) {
        for (int q = 0; q < SC_P; q++) {
            const int last = path_off[q] + (path_len[q] > 0 ? path_len[q] - 1 : 0);
            const bool near = (q == 0 && s >= 2) || (q == 2 && s >= 5) || q == 3 || q == 4;
            state[4 * q] = near ? path[3 * last] + 0.3 : 40.0 + 30.0 * rnd(); state[4 * q + 1] = near ? path[3 * last + 1] : 30.0 * rnd();
            state[4 * q + 2] = q == 3 ? 0.5 : 0.05; state[4 * q + 3] = rnd();      // agent 3 is there, but too fast
            applied[2 * q] = 0.1 + rnd(); applied[2 * q + 1] = 0.1 + rnd();
            goal_len[q] = path_len[q];
            target[q] = q == 4 ? 3 : path_len[q] - 2;                               // agent 4 is there, but its target index is not
        }
        retire_ref_step(SC_P, state.data(), applied.data(), path.data(), path_off, path_len, target.data(), goal_len.data(), &r);
        for (int q = 0; q < SC_P; q++) { out[o++] = done[q]; out[o++] = driven[q]; out[o++] = applied[2 * q]; out[o++] = applied[2 * q + 1]; }
    }
}

#ifdef RETIRE_REF_MAIN
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<double> out((size_t)retire_ref_selfcase_size());
    retire_ref_selfcase(out.data());
    FILE *g = fopen(argv[1], "wb");
    if (!g) return 3;
    fwrite(out.data(), sizeof(double), out.size(), g);
    fclose(g);
    return 0;
}
#endif
