// Host build of csrc/mpcx_record_core.h and csrc/mpcx_retire_core.h WITH A SCENE (mpcx_scene: departure): the record rule whose clearance
// leaves absent pool rows out, and the retire rule that sets the arrived agent's word of the mask.  The GPU's record_kernel and retire_kernel
// compile the very same headers.  Test infrastructure (tests/test_scene_cpu.py), also run under the sanitizers; never loaded by the product.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_retire_core.h"

static mpcx::RecordArgs record_args(const mpcx_interaction_params *ip, int P, int T, const double *state, const double *applied, const double *x_sol,
                                    const double *path_xyyaw, const int32_t *path_off, const int32_t *path_len, const int32_t *target_ind,
                                    const int32_t *cut_len, const int32_t *traj_idx, const int32_t *hit_idx, const int32_t *status,
                                    const int32_t *iters, int n_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt,
                                    const int32_t *obs_skip, const mpcx_run_log *log, const int32_t *goal_len, const int32_t *done,
                                    const int32_t *absent) {
    mpcx::RecordArgs a{};
    a.P = P; a.n_pool = n_pool; a.x_stride = 4 * (int64_t)(T + 1);
    a.radius = ip->radius;
    for (int k = 0; k < 4; k++) a.cc[k] = ip->circle_centers[k];
    a.state = state; a.applied = applied; a.x_sol = x_sol; a.path_xyyaw = path_xyyaw; a.obs6 = obs6;
    a.path_off = path_off; a.path_len = path_len; a.target_ind = target_ind; a.cut_len = cut_len; a.traj_idx = traj_idx;
    a.hit_idx = hit_idx; a.status = status; a.iters = iters; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip;
    if (log) a.log = *log;
    a.goal_len = goal_len; a.done = done; a.absent = absent;
    return a;
}

// rec_clearance of agent q alone: pool[n_pool][6], the agent's window and own row, the mask or NULL
extern "C" double scene_ref_clearance(const mpcx_interaction_params *ip, int n_pool, const double *obs6, int off, int cnt, int own,
                                      const int32_t *absent) {
    const int32_t o = off, c = cnt, s = own;
    mpcx::RecordArgs a = record_args(ip, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, n_pool, obs6, &o, &c, &s, nullptr, nullptr, nullptr, absent);
    return mpcx::rec_clearance(a, 0);
}

// one step's record for P agents as record_kernel runs it under retirement with a scene: a retired agent (done[q] != 0) is skipped
extern "C" void scene_ref_record_step(const mpcx_interaction_params *ip, int P, int T, const double *state, const double *applied, const double *x_sol,
                                      const double *path_xyyaw, const int32_t *path_off, const int32_t *path_len, const int32_t *target_ind,
                                      const int32_t *cut_len, const int32_t *traj_idx, const int32_t *hit_idx, const int32_t *status,
                                      const int32_t *iters, int n_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt,
                                      const int32_t *obs_skip, const mpcx_run_log *log, const int32_t *goal_len, const int32_t *done,
                                      const int32_t *absent) {
    const mpcx::RecordArgs a = record_args(ip, P, T, state, applied, x_sol, path_xyyaw, path_off, path_len, target_ind, cut_len, traj_idx, hit_idx,
                                           status, iters, n_pool, obs6, obs_off, obs_cnt, obs_skip, log, goal_len, done, absent);
    for (int q = 0; q < P; q++) {
        if (done && done[q] != 0) continue;
        double f[mpcx::REC_F64];
        int32_t w[mpcx::REC_I32];
        const int32_t s = mpcx::record_agent(a, q, f, w);
        if (s >= log->capacity) continue;
        const size_t row = (size_t)s * (size_t)P + (size_t)q;
        for (int k = 0; k < mpcx::REC_F64; k++) log->rows_f64[mpcx::REC_F64 * row + k] = f[k];
        for (int k = 0; k < mpcx::REC_I32; k++) log->rows_i32[mpcx::REC_I32 * row + k] = w[k];
    }
}

// one step's retirement for P agents with a scene (or scene = NULL: retirement alone), the arguments of retire_kernel with HOST pointers;
// returns the number of agents that arrived
extern "C" int scene_ref_retire_step(int P, const double *state, double *applied, const double *path_xyyaw, const int32_t *path_off,
                                     const int32_t *path_len, const int32_t *target_ind, const int32_t *goal_len, const mpcx_retire *r,
                                     const mpcx_scene *scene, const int32_t *own_row) {
    mpcx::RetireArgs a{P, state, path_xyyaw, applied, path_off, path_len, target_ind, goal_len, *r};
    if (scene) { a.absent = scene->absent; a.own_row = own_row; a.n_rows = scene->n_rows; }
    int n = 0;
    for (int q = 0; q < P; q++) n += mpcx::retire_agent(a, q) ? 1 : 0;
    return n;
}

// layout of mpcx_scene as the header's own compiler has it: sizeof, the offsets of its fields in order; then the sizes of the structs that
// departure travels beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire
extern "C" void scene_ref_layout(int64_t *out8) {
    const size_t v[8] = {sizeof(mpcx_scene), offsetof(mpcx_scene, absent), offsetof(mpcx_scene, n_rows), offsetof(mpcx_scene, reserved),
                         sizeof(mpcx_closed_loop), sizeof(mpcx_closed_loop_opts), sizeof(mpcx_run_log), sizeof(mpcx_retire)};
    for (int i = 0; i < 8; i++) out8[i] = (int64_t)v[i];
}

// A self-contained case on seeded pseudo-random data: 5 agents in two windows of a 9-row pool (rows 7 and 8 are scripted cars; row 8 is
// hidden from the start), arrivals at different steps, one agent whose own row lies outside the pool (its arrival writes nothing), a window
// that reaches beyond the pool.  out: per step the mask (SC_POOL), then per agent (done, clearance with the mask, clearance without it).
enum { SC_P = 5, SC_STEPS = 7, SC_POOL = 9, SC_NPTS = 20 };
extern "C" int scene_ref_selfcase_size(void) { return SC_STEPS * (SC_POOL + 3 * SC_P); }
extern "C" void scene_ref_selfcase(double *out) {
    uint64_t seed = 2024;
    auto rnd = [&seed]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
    mpcx_interaction_params ip = {};
    ip.radius = 1.0; ip.circle_centers[0] = 0.5; ip.circle_centers[2] = 2.0;
    std::vector<double> path(3 * SC_NPTS), state(4 * SC_P), applied(2 * SC_P), obs6(6 * SC_POOL);
    for (int i = 0; i < SC_NPTS; i++) { path[3 * i] = 0.5 * i; path[3 * i + 1] = 0.1 * i; path[3 * i + 2] = 0.2; }
    const int32_t path_off[SC_P] = {0, 0, 10, 10, 0}, path_len[SC_P] = {10, 10, 10, 10, 20};
    const int32_t obs_off[SC_P] = {0, 0, 3, 3, 3}, obs_cnt[SC_P] = {3, 3, 9, 6, 6}, own[SC_P] = {0, 1, 3, 4, 99};
    std::vector<int32_t> target(SC_P), goal_len(SC_P), done(SC_P, 0), driven(SC_P, 0), absent(SC_POOL, 0);
    absent[8] = 1;
    mpcx_retire r = {done.data(), driven.data(), 1.5, 0.1389};
    mpcx_scene sc = {absent.data(), SC_POOL, 0};
    size_t o = 0;
    for (int s = 0; s < SC_STEPS; s++) {
        for (int k = 0; k < 6 * SC_POOL; k++) obs6[k] = (k % 6 == 3 ? 6.0 : 12.0) * rnd() - (k % 6 == 3 ? 3.0 : 0.0);
        for (int q = 0; q < SC_P; q++) {
            const int last = path_off[q] + path_len[q] - 1;
            const bool near = (q == 0 && s >= 1) || (q == 3 && s >= 3) || (q == 4 && s >= 4);
            state[4 * q] = near ? path[3 * last] + 0.3 : 40.0 + 30.0 * rnd(); state[4 * q + 1] = near ? path[3 * last + 1] : 30.0 * rnd();
            state[4 * q + 2] = 0.05; state[4 * q + 3] = rnd();
            applied[2 * q] = 0.1 + rnd(); applied[2 * q + 1] = 0.1 + rnd();
            goal_len[q] = path_len[q]; target[q] = path_len[q] - 2;
        }
        for (int q = 0; q < SC_P; q++) {
            out[o + SC_POOL + 3 * q + 1] = scene_ref_clearance(&ip, SC_POOL, obs6.data(), obs_off[q], obs_cnt[q], own[q], absent.data());
            out[o + SC_POOL + 3 * q + 2] = scene_ref_clearance(&ip, SC_POOL, obs6.data(), obs_off[q], obs_cnt[q], own[q], nullptr);
        }
        scene_ref_retire_step(SC_P, state.data(), applied.data(), path.data(), path_off, path_len, target.data(), goal_len.data(), &r, &sc, own);
        for (int k = 0; k < SC_POOL; k++) out[o + k] = absent[k];
        for (int q = 0; q < SC_P; q++) out[o + SC_POOL + 3 * q] = done[q];
        o += SC_POOL + 3 * SC_P;
    }
}

#ifdef SCENE_REF_MAIN
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<double> out((size_t)scene_ref_selfcase_size());
    scene_ref_selfcase(out.data());
    FILE *g = fopen(argv[1], "wb");
    if (!g) return 3;
    fwrite(out.data(), sizeof(double), out.size(), g);
    fclose(g);
    return 0;
}
#endif
