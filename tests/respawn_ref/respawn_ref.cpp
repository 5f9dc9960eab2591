// Host build of csrc/mpcx_respawn_core.h: the respawn rule (episode record, slot reset, hand-over to the admission gate) as a plain loop over
// host arrays.  The GPU's respawn_kernel compiles the very same header.  Test infrastructure (tests/test_respawn_cpu.py), also run under the
// sanitizers; never loaded by the product.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_respawn_core.h"

// One step's respawn for P agents, the arguments of the kernel with HOST pointers.  u_len = 2 T doubles of u_sol per agent; prev_len and log
// may be NULL.  backwards != 0: the lanes are visited from the last to the first (the outcome must not depend on it).  Returns the number of
// agents that arrived.
extern "C" int respawn_ref_step(int P, int n_pool, int u_len, double *state, double *applied, double *u_sol, int32_t *traj_idx,
                                int32_t *target_ind, int32_t *cut_len, int32_t *iters, int32_t *prev_len, const int32_t *own_row,
                                const mpcx_run_log *log, const mpcx_retire *retire, const mpcx_admit *admit, const mpcx_respawn *rs,
                                int backwards) {
    mpcx::RespawnArgs a = {};
    a.P = P; a.n_pool = n_pool; a.u_len = u_len;
    a.has_log = log ? 1 : 0; a.has_prev_len = prev_len ? 1 : 0;
    a.state = state; a.applied = applied; a.u_sol = u_sol;
    a.traj_idx = traj_idx; a.target_ind = target_ind; a.cut_len = cut_len; a.iters = iters; a.prev_len = prev_len;
    a.own_row = own_row;
    a.done = retire->done; a.steps_driven = retire->steps_driven;
    a.ad = *admit;
    if (log) a.log = *log;
    a.rs = *rs;
    int got = 0;
    for (int k = 0; k < P; k++) {
        const int q = backwards ? P - 1 - k : k;
        if (a.done[q] == 0) continue;           // (the kernel's early exit)
        got += mpcx::respawn_agent(a, q) ? 1 : 0;
    }
    return got;
}

// layout of mpcx_respawn as the header's own compiler has it: sizeof, the offsets of its fields in order; then the sizes of the structs that
// respawn travels beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene, mpcx_admit
extern "C" void respawn_ref_layout(int64_t *out15) {
    const size_t v[15] = {sizeof(mpcx_respawn), offsetof(mpcx_respawn, generations), offsetof(mpcx_respawn, reserved),
                          offsetof(mpcx_respawn, start_state), offsetof(mpcx_respawn, start_idx), offsetof(mpcx_respawn, due),
                          offsetof(mpcx_respawn, served), offsetof(mpcx_respawn, ep_i32), offsetof(mpcx_respawn, ep_f64),
                          sizeof(mpcx_closed_loop), sizeof(mpcx_closed_loop_opts), sizeof(mpcx_run_log), sizeof(mpcx_retire), sizeof(mpcx_scene),
                          sizeof(mpcx_admit)};
    for (int i = 0; i < 15; i++) out15[i] = (int64_t)v[i];
}

#ifdef RESPAWN_REF_MAIN
// Runs the cases of a file written by tests/test_respawn_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_pool, u_len, G, has_log, has_prev_len, backwards, steps
//   f64: state (P,4), applied (P,2), u_sol (P,u_len), start_state (P,4), ep_f64 (P,G,2), min_clearance (P)
//   i32: traj_idx, target_ind, cut_len, iters, prev_len, own_row, done, steps_driven, wait, entered_step (P each), clock (1), start_idx (P),
//        due (P,G), served (P), ep_i32 (P,G,8), steps, goal_step, contact_step, flags (P each)
// (prev_len and the log's words are in the file whatever the flags say.)  out per case and step: the mutable words in the same order --
// state, applied, u_sol, ep_f64, min_clearance as f64, then traj_idx, target_ind, cut_len, iters, prev_len, steps_driven, wait, entered_step,
// served, ep_i32, steps, goal_step, contact_step, flags and the number arrived as int32.
template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T>
static void wr(FILE *g, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[8];
    while (fread(h, sizeof(int32_t), 8, f) == 8) {
        const size_t P = (size_t)h[0], G = (size_t)h[3];
        const int n_pool = h[1], u_len = h[2], has_log = h[4], has_prev = h[5], backwards = h[6], steps = h[7];
        std::vector<double> state, applied, u, start_state, ep_f64, minc;
        std::vector<int32_t> traj, target, cut, iters, prev, own, done, driven, wait, entered, clock, start_idx, due, served, ep_i32, lsteps, goal,
            contact, flags;
        if (!rd(f, state, 4 * P) || !rd(f, applied, 2 * P) || !rd(f, u, (size_t)u_len * P) || !rd(f, start_state, 4 * P) || !rd(f, ep_f64, 2 * G * P) ||
            !rd(f, minc, P) || !rd(f, traj, P) || !rd(f, target, P) || !rd(f, cut, P) || !rd(f, iters, P) || !rd(f, prev, P) || !rd(f, own, P) ||
            !rd(f, done, P) || !rd(f, driven, P) || !rd(f, wait, P) || !rd(f, entered, P) || !rd(f, clock, 1) || !rd(f, start_idx, P) ||
            !rd(f, due, G * P) || !rd(f, served, P) || !rd(f, ep_i32, 8 * G * P) || !rd(f, lsteps, P) || !rd(f, goal, P) || !rd(f, contact, P) ||
            !rd(f, flags, P))
            return 5;
        mpcx_run_log log = {};
        log.steps = lsteps.data(); log.goal_step = goal.data(); log.contact_step = contact.data(); log.flags = flags.data();
        log.min_clearance = minc.data();
        mpcx_retire retire = {done.data(), driven.data(), 1.5, 0.1389};
        mpcx_admit admit = {wait.data(), entered.data(), clock.data(), 0, 0.0};
        mpcx_respawn rs = {(int32_t)G, 0, start_state.data(), start_idx.data(), due.data(), served.data(), ep_i32.data(), ep_f64.data()};
        for (int s = 0; s < steps; s++) {
            const int32_t got = respawn_ref_step((int)P, n_pool, u_len, state.data(), applied.data(), u.data(), traj.data(), target.data(), cut.data(),
                                                 iters.data(), has_prev ? prev.data() : nullptr, own.data(), has_log ? &log : nullptr, &retire,
                                                 &admit, &rs, backwards);
            wr(g, state); wr(g, applied); wr(g, u); wr(g, ep_f64); wr(g, minc);
            wr(g, traj); wr(g, target); wr(g, cut); wr(g, iters); wr(g, prev); wr(g, driven); wr(g, wait); wr(g, entered); wr(g, served);
            wr(g, ep_i32); wr(g, lsteps); wr(g, goal); wr(g, contact); wr(g, flags);
            fwrite(&got, sizeof(int32_t), 1, g);
            clock[0] += 1;          // the next step's admission stage would have advanced it
        }
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
