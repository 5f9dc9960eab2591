// Host build of csrc/mpcx_record_core.h (the run log's record rule of one agent and step; the GPU's record_kernel compiles the very same
// header): test infrastructure that feeds it the reference's recorded runs and lets the sanitizers see it.  Never loaded by the product path.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_record_core.h"

// one step's record for P agents, the arguments of mpcx_record_step_batch with HOST pointers (T: the horizon, which the library takes
// from its context); rows are stored as record_kernel stores them ([step][agent][8], dropped beyond the capacity)
extern "C" void record_ref_step(const mpcx_interaction_params *ip, int P, int T, const double *state, const double *applied, const double *x_sol,
                                const double *path_xyyaw, const int32_t *path_off, const int32_t *path_len, const int32_t *target_ind,
                                const int32_t *cut_len, const int32_t *traj_idx, const int32_t *hit_idx, const int32_t *status,
                                const int32_t *iters, int n_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt,
                                const int32_t *obs_skip, const mpcx_run_log *log) {
    mpcx::RecordArgs a;
    a.P = P; a.n_pool = n_pool; a.x_stride = 4 * (int64_t)(T + 1);
    a.radius = ip->radius;
    for (int k = 0; k < 4; k++) a.cc[k] = ip->circle_centers[k];
    a.state = state; a.applied = applied; a.x_sol = x_sol; a.path_xyyaw = path_xyyaw; a.obs6 = obs6;
    a.path_off = path_off; a.path_len = path_len; a.target_ind = target_ind; a.cut_len = cut_len; a.traj_idx = traj_idx;
    a.hit_idx = hit_idx; a.status = status; a.iters = iters; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip;
    a.log = *log;
    for (int q = 0; q < P; q++) {
        double f[mpcx::REC_F64];
        int32_t w[mpcx::REC_I32];
        const int32_t s = mpcx::record_agent(a, q, f, w);
        if (s >= log->capacity) continue;
        const size_t row = (size_t)s * (size_t)P + (size_t)q;
        for (int k = 0; k < mpcx::REC_F64; k++) log->rows_f64[mpcx::REC_F64 * row + k] = f[k];
        for (int k = 0; k < mpcx::REC_I32; k++) log->rows_i32[mpcx::REC_I32 * row + k] = w[k];
    }
}

// layout of mpcx_run_log as the header's own compiler has it: sizeof, then the offsets of its fields in order; out[12] = sizeof(mpcx_closed_loop)
extern "C" void record_ref_layout(int64_t *out13) {
    const size_t v[13] = {sizeof(mpcx_run_log), offsetof(mpcx_run_log, capacity), offsetof(mpcx_run_log, reserved), offsetof(mpcx_run_log, goal_dis),
                          offsetof(mpcx_run_log, stop_speed), offsetof(mpcx_run_log, rows_f64), offsetof(mpcx_run_log, rows_i32),
                          offsetof(mpcx_run_log, steps), offsetof(mpcx_run_log, goal_step), offsetof(mpcx_run_log, contact_step),
                          offsetof(mpcx_run_log, flags), offsetof(mpcx_run_log, min_clearance), sizeof(mpcx_closed_loop)};
    for (int i = 0; i < 13; i++) out13[i] = (int64_t)v[i];
}

// A self-contained case that walks every branch of the rule -- windows with nobody else, empty, longer than the rule walks and partly
// outside the pool, an agent without a row of its own, failed solves, target indices outside the path, an empty path, arrivals, contacts
// after separation, a capacity smaller than the run -- on seeded pseudo-random data.  out: everything the log holds, as doubles
// (n_out = record_ref_selfcase_size()).  The sanitizer build runs it as a program, the plain build returns the same numbers.
enum { SC_P = 7, SC_STEPS = 9, SC_CAP = 4, SC_T = 3, SC_POOL = 24, SC_NPTS = 40 };
extern "C" int record_ref_selfcase_size(void) { return SC_CAP * SC_P * 16 + SC_P * 5; }
extern "C" void record_ref_selfcase(double *out) {
    uint64_t seed = 12345;
    auto rnd = [&seed]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
    mpcx_interaction_params ip = {};
    ip.radius = 1.0; ip.circle_centers[0] = 0.5; ip.circle_centers[2] = 2.0;
    std::vector<double> path(3 * SC_NPTS), state(4 * SC_P), applied(2 * SC_P), x_sol(4 * (SC_T + 1) * SC_P), obs6(6 * SC_POOL);
    for (int i = 0; i < SC_NPTS; i++) { path[3 * i] = 0.5 * i; path[3 * i + 1] = 0.1 * i; path[3 * i + 2] = 0.2; }
    const int32_t path_off[SC_P] = {0, 0, 10, 10, 20, 0, 38}, path_len[SC_P] = {10, 10, 10, 10, 20, 40, 0};
    const int32_t obs_off[SC_P] = {0, 0, 4, 4, 4, 20, 8}, obs_cnt[SC_P] = {2, 2, 20, 1, 0, 9, 3}, obs_skip[SC_P] = {0, 1, 5, 4, 6, 21, 99};
    std::vector<int32_t> target(SC_P), cut(SC_P), tidx(SC_P), hit(SC_P), status(SC_P), iters(SC_P);
    std::vector<double> rf(SC_CAP * SC_P * 8, -7.0), mc(SC_P, INFINITY);
    std::vector<int32_t> ri(SC_CAP * SC_P * 8, -7), steps(SC_P, 0), goal(SC_P, -1), contact(SC_P, -1), flags(SC_P, 0);
    mpcx_run_log log = {SC_CAP, 0, 1.5, 0.1389, rf.data(), ri.data(), steps.data(), goal.data(), contact.data(), flags.data(), mc.data()};
    for (int s = 0; s < SC_STEPS; s++) {
        for (int r = 0; r < SC_POOL; r++) {
            // rows 0 and 1 drift apart, then row 1 comes back onto row 0 (a contact after separation); the others are scattered
            double *o = &obs6[6 * r];
            o[0] = r < 2 ? (r ? (s < 5 ? 2.0 * s : 2.0 * (8 - s)) : 0.0) : 40.0 * rnd();
            o[1] = r < 2 ? 0.0 : 40.0 * rnd();
            o[2] = rnd(); o[3] = r < 2 ? 0.0 : 6.0 * rnd() - 3.0; o[4] = rnd(); o[5] = rnd();
        }
        for (int q = 0; q < SC_P; q++) {
            const int last = path_off[q] + (path_len[q] > 0 ? path_len[q] - 1 : 0);
            const bool there = (q == 2 && s >= 3) || (q == 3 && s >= 6);
            state[4 * q] = there ? path[3 * last] + 0.3 : 30.0 * rnd(); state[4 * q + 1] = there ? path[3 * last + 1] : 30.0 * rnd();
            state[4 * q + 2] = there ? 0.05 : 1.0 + rnd(); state[4 * q + 3] = rnd();
            applied[2 * q] = rnd(); applied[2 * q + 1] = rnd();
            for (int k = 0; k < 4 * (SC_T + 1); k++) x_sol[4 * (SC_T + 1) * q + k] = 20.0 * rnd();
            cut[q] = path_len[q];
            target[q] = there ? path_len[q] - 2 : (q == 5 && s == 2 ? 40 : (q == 5 && s == 3 ? -1 : (int32_t)(rnd() * (path_len[q] > 0 ? path_len[q] : 1))));
            tidx[q] = (int32_t)(100 * rnd()); hit[q] = (int32_t)(100 * rnd()) - 3; iters[q] = (int32_t)(20 * rnd());
            status[q] = (q == 1 && s % 3 == 1) ? 2 : 0;
        }
        record_ref_step(&ip, SC_P, SC_T, state.data(), applied.data(), x_sol.data(), path.data(), path_off, path_len, target.data(), cut.data(),
                        tidx.data(), hit.data(), status.data(), iters.data(), SC_POOL, obs6.data(), obs_off, obs_cnt, obs_skip, &log);
    }
    size_t o = 0;
    for (size_t r = 0; r < (size_t)SC_CAP * SC_P; r++) {
        for (int k = 0; k < 8; k++) out[o++] = rf[8 * r + k];
        for (int k = 0; k < 8; k++) out[o++] = (double)ri[8 * r + k];
    }
    for (int q = 0; q < SC_P; q++) {
        out[o++] = steps[q]; out[o++] = goal[q]; out[o++] = contact[q]; out[o++] = flags[q]; out[o++] = mc[q];
    }
}

#ifdef RECORD_REF_MAIN
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<double> out((size_t)record_ref_selfcase_size());
    record_ref_selfcase(out.data());
    FILE *g = fopen(argv[1], "wb");
    if (!g) return 3;
    fwrite(out.data(), sizeof(double), out.size(), g);
    fclose(g);
    return 0;
}
#endif
