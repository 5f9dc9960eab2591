// Host build of csrc/mpcx_admit_core.h: the admission rule (snapshot of the pool's poses and tags, then the gate) as plain loops over host
// arrays.  The GPU's admit_snapshot_kernel and admit_gate_kernel compile the very same header.  Test infrastructure
// (tests/test_admit_cpu.py), also run under the sanitizers; never loaded by the product.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_admit_core.h"

// One step's admission for P agents and n_actors scripted cars, the arguments of the kernels with HOST pointers.
// backwards != 0: both passes visit their lanes from the last to the first (the outcome must not depend on it).
// tab_pose (n_pool,3), tab_tag (n_pool): the table, caller-owned, tags zeroed by the caller as the library zeroes them.
// rows6 (n_actors,6) or NULL: the get() row of every actor as the snapshot computed it.  Returns the number of agents admitted.
extern "C" int admit_ref_step(const mpcx_interaction_params *ip, int P, const double *state, const int32_t *obs_off, const int32_t *obs_cnt,
                              const int32_t *own_row, int32_t *done, int n_pool, int32_t *absent, int n_actors,
                              const mpcx_traffic_actor *actors, const double *actor_state, const double *tape, int64_t tape_rows,
                              const int32_t *actor_row, const mpcx_admit *admit, int backwards, double *tab_pose, int32_t *tab_tag,
                              double *rows6) {
    mpcx::AdmitArgs a{};
    a.P = P; a.n_pool = n_pool; a.n_actors = n_actors;
    a.radius = ip->radius;
    for (int k = 0; k < 4; k++) a.cc[k] = ip->circle_centers[k];
    a.state = state; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.own_row = own_row; a.done = done; a.absent = absent;
    a.actors = actors; a.actor_state = actor_state; a.tape = tape; a.tape_rows = tape ? tape_rows : 0; a.actor_row = actor_row;
    a.ad = *admit;
    a.tab_pose = tab_pose; a.tab_tag = tab_tag;
    const int n = P + n_actors;
    mpcx::admit_tick(a);
    for (int k = 0; k < n; k++) {
        const int i = backwards ? n - 1 - k : k;
        if (i < P) mpcx::admit_snapshot_agent(a, i);
        else mpcx::admit_snapshot_actor(a, i - P, rows6 ? rows6 + 6 * (size_t)(i - P) : nullptr);
    }
    int got = 0;
    for (int k = 0; k < P; k++) {
        const int q = backwards ? P - 1 - k : k;
        if (a.ad.wait[q] < 0) continue;         // (the kernel's early exit)
        got += mpcx::admit_gate_agent(a, q) ? 1 : 0;
    }
    return got;
}

// traffic_get_step alone on a COPY of the actor's state: the row the traffic stage emits in this step
extern "C" void admit_ref_actor_row(const mpcx_traffic_actor *actor, const double *state4, const double *tape, int64_t tape_rows, double *row6) {
    double st[4] = {state4[0], state4[1], state4[2], state4[3]};
    mpcx::traffic_get_step(*actor, st, tape, tape ? tape_rows : 0, row6);
}

// layout of mpcx_admit as the header's own compiler has it: sizeof, the offsets of its fields in order; then the sizes of the structs that
// admission travels beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene
extern "C" void admit_ref_layout(int64_t *out11) {
    const size_t v[11] = {sizeof(mpcx_admit), offsetof(mpcx_admit, wait), offsetof(mpcx_admit, entered_step), offsetof(mpcx_admit, clock),
                          offsetof(mpcx_admit, reserved), offsetof(mpcx_admit, gap), sizeof(mpcx_closed_loop), sizeof(mpcx_closed_loop_opts),
                          sizeof(mpcx_run_log), sizeof(mpcx_retire), sizeof(mpcx_scene)};
    for (int i = 0; i < 11; i++) out11[i] = (int64_t)v[i];
}

#ifdef ADMIT_REF_MAIN
// Runs the cases of a file written by tests/test_admit_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_pool, n_actors, tape_rows, backwards, steps;  double gap, radius, cc[4];
//   state (P,4) f64; obs_off, obs_cnt, own_row, done, wait, entered_step (P each) i32; absent (n_pool) i32; clock i32;
//   actors (n_actors structs); actor_state (n_actors,4) f64; actor_row (n_actors) i32; tape (tape_rows,6) f64
// out per case and step: done, wait, entered_step (P each), absent (n_pool), clock, admitted -- as int32.
template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[6];
    while (fread(h, sizeof(int32_t), 6, f) == 6) {
        const int P = h[0], n_pool = h[1], n_actors = h[2], tape_rows = h[3], backwards = h[4], steps = h[5];
        double d[6];
        if (fread(d, sizeof(double), 6, f) != 6) return 4;
        std::vector<double> state, actor_state, tape;
        std::vector<int32_t> obs_off, obs_cnt, own, done, wait, entered, absent, clock, actor_row;
        std::vector<mpcx_traffic_actor> actors;
        if (!rd(f, state, 4 * (size_t)P) || !rd(f, obs_off, P) || !rd(f, obs_cnt, P) || !rd(f, own, P) || !rd(f, done, P) || !rd(f, wait, P) ||
            !rd(f, entered, P) || !rd(f, absent, n_pool) || !rd(f, clock, 1) || !rd(f, actors, n_actors) || !rd(f, actor_state, 4 * (size_t)n_actors) ||
            !rd(f, actor_row, n_actors) || !rd(f, tape, 6 * (size_t)tape_rows))
            return 5;
        mpcx_interaction_params ip = {};
        ip.radius = d[1];
        for (int k = 0; k < 4; k++) ip.circle_centers[k] = d[2 + k];
        mpcx_admit ad = {wait.data(), entered.data(), clock.data(), 0, d[0]};
        std::vector<double> pose(3 * (size_t)n_pool);
        std::vector<int32_t> tag((size_t)n_pool, 0);
        for (int s = 0; s < steps; s++) {
            const int32_t got = admit_ref_step(&ip, P, state.data(), obs_off.data(), obs_cnt.data(), own.data(), done.data(), n_pool, absent.data(),
                                               n_actors, actors.data(), actor_state.data(), tape_rows ? tape.data() : nullptr, tape_rows,
                                               actor_row.data(), &ad, backwards, pose.data(), tag.data(), nullptr);
            fwrite(done.data(), sizeof(int32_t), P, g); fwrite(wait.data(), sizeof(int32_t), P, g); fwrite(entered.data(), sizeof(int32_t), P, g);
            fwrite(absent.data(), sizeof(int32_t), n_pool, g); fwrite(clock.data(), sizeof(int32_t), 1, g); fwrite(&got, sizeof(int32_t), 1, g);
        }
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
