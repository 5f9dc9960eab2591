// Host build of csrc/mpcx_intent_core.h: the shared-plans rule as a plain loop over host arrays.  The GPU's intent_kernel compiles the very
// same header.  Test infrastructure (tests/test_intent_cpu.py, tests/test_gpu_intent.py), also run under the sanitizers as a stand-alone
// program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_intent_core.h"

// One step's shared-plans stage for P agents with plans of T columns, the arguments of the kernel with HOST pointers (done and absent may
// be null).  backwards != 0: the lanes are visited from the last to the first (the outcome must not depend on it).  Writes frames (P) and
// the pred_steps frames of every sharing agent's own row of pred (n_pool x pred_steps x 4); returns the number of agents taken from
// their plans.
extern "C" int intent_ref_step(int P, int T, int n_pool, int pred_steps, double dt, double L, const double *circle_centers4, const double *state,
                               const double *u_sol, const int32_t *status, const int32_t *obs_skip, const int32_t *done, const int32_t *absent,
                               const int32_t *share, int32_t *frames, double *pred, int backwards) {
    mpcx::IntentArgs a = {};
    a.ip.pred_steps = pred_steps; a.ip.dt = dt; a.ip.L = L;
    for (int k = 0; k < 4; k++) a.ip.circle_centers[k] = circle_centers4[k];
    a.P = P; a.T = T; a.n_pool = n_pool;
    a.has_done = done != nullptr; a.has_absent = absent != nullptr;
    a.state = state; a.u_sol = u_sol; a.status = status; a.obs_skip = obs_skip; a.done = done; a.absent = absent; a.pred = pred;
    a.in = {share, frames, P, 0};
    int got = 0;
    for (int k = 0; k < P; k++) got += mpcx::intent_agent(a, backwards ? P - 1 - k : k) > 0 ? 1 : 0;
    return got;
}

// layout of mpcx_intent as the header's own compiler has it: sizeof, the offsets of its four fields in order; then the sizes of the structs
// that the stage travels beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene,
// mpcx_admit, mpcx_respawn, mpcx_routes, mpcx_precedence, mpcx_signals, mpcx_actuation, mpcx_advice, mpcx_interaction_params
extern "C" void intent_ref_layout(int64_t *out18) {
#define OFF(f) (int64_t)offsetof(mpcx_intent, f)
    const int64_t v[18] = {(int64_t)sizeof(mpcx_intent), OFF(share), OFF(frames), OFF(n_rows), OFF(reserved),
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes), (int64_t)sizeof(mpcx_precedence), (int64_t)sizeof(mpcx_signals),
                           (int64_t)sizeof(mpcx_actuation), (int64_t)sizeof(mpcx_advice), (int64_t)sizeof(mpcx_interaction_params)};
#undef OFF
    for (int i = 0; i < 18; i++) out18[i] = v[i];
}

#ifdef INTENT_REF_MAIN
// Runs the cases of a file written by tests/test_intent_cpu.py and writes every case's words back.  Per case:
//   int32 P, T, n_pool, pred_steps, has_done, has_absent, backwards, 0; double dt, L, circle_centers (4); double state (4 P), u_sol (2 T P);
//   int32 status, obs_skip, share (P each), done (P, only with has_done), absent (n_pool, only with has_absent); double pred (4 pred_steps
//   n_pool)
// out per case: frames (P int32), pred (4 pred_steps n_pool doubles) and the number of agents taken from their plans, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static bool rd(FILE *f, std::vector<double> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(double), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[8];
    while (fread(h, sizeof(int32_t), 8, f) == 8) {
        const size_t P = (size_t)h[0], T = (size_t)h[1], np = (size_t)h[2], S = (size_t)h[3];
        double d[6];
        if (fread(d, sizeof(double), 6, f) != 6) return 4;
        std::vector<double> state, u, pred;
        std::vector<int32_t> status, skip, share, done, absent, frames(P);
        if (!rd(f, state, 4 * P) || !rd(f, u, 2 * T * P) || !rd(f, status, P) || !rd(f, skip, P) || !rd(f, share, P) || !rd(f, done, h[4] ? P : 0) ||
            !rd(f, absent, h[5] ? np : 0) || !rd(f, pred, 4 * S * np))
            return 5;
        const int32_t got = intent_ref_step((int)P, (int)T, (int)np, (int)S, d[0], d[1], d + 2, state.data(), u.data(), status.data(), skip.data(),
                                            h[4] ? done.data() : nullptr, h[5] ? absent.data() : nullptr, share.data(), frames.data(), pred.data(),
                                            h[6]);
        if (P) fwrite(frames.data(), sizeof(int32_t), P, g);
        if (!pred.empty()) fwrite(pred.data(), sizeof(double), pred.size(), g);
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
