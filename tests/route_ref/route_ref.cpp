// Host build of csrc/mpcx_route_core.h: the routed respawn rule (the respawn rule, then the episode's route word and the next vehicle's route,
// start pose and index) and the per-movement summary as plain loops over host arrays.  The GPU's respawn_route_kernel and summary_kernel
// compile the very same header.  Test infrastructure (tests/test_route_cpu.py), also run under the sanitizers; never loaded by the product.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_route_core.h"

// One step's routed respawn for P agents, the arguments of the kernel with HOST pointers (as respawn_ref_step, plus the routes struct).
// backwards != 0: the lanes are visited from the last to the first (the outcome must not depend on it).  Returns the number of agents that
// arrived.
extern "C" int route_ref_step(int P, int n_pool, int u_len, double *state, double *applied, double *u_sol, int32_t *traj_idx,
                              int32_t *target_ind, int32_t *cut_len, int32_t *iters, int32_t *prev_len, const int32_t *own_row,
                              const mpcx_run_log *log, const mpcx_retire *retire, const mpcx_admit *admit, const mpcx_respawn *rs,
                              const mpcx_routes *rt, int backwards) {
    mpcx::RouteArgs a = {};
    a.r.P = P; a.r.n_pool = n_pool; a.r.u_len = u_len;
    a.r.has_log = log ? 1 : 0; a.r.has_prev_len = prev_len ? 1 : 0;
    a.r.state = state; a.r.applied = applied; a.r.u_sol = u_sol;
    a.r.traj_idx = traj_idx; a.r.target_ind = target_ind; a.r.cut_len = cut_len; a.r.iters = iters; a.r.prev_len = prev_len;
    a.r.own_row = own_row;
    a.r.done = retire->done; a.r.steps_driven = retire->steps_driven;
    a.r.ad = *admit;
    if (log) a.r.log = *log;
    a.r.rs = *rs;
    a.rt = *rt;
    int got = 0;
    for (int k = 0; k < P; k++) {
        const int q = backwards ? P - 1 - k : k;
        if (a.r.done[q] == 0) continue;         // (the kernel's early exit)
        got += mpcx::route_agent(a, q) ? 1 : 0;
    }
    return got;
}

// mpcx_episode_summary on host arrays: per instance (A consecutive slots) and route, over the finished episodes whose word 7 is the route
extern "C" void route_ref_summary(int P, int A, int G, int R, const int32_t *served, const int32_t *ep_i32, const double *ep_f64,
                                  int64_t *out_i64, double *out_f64) {
    for (int b = 0; b < P / A; b++)
        for (int r = 0; r < R; r++) {
            int64_t acc[4] = {0, 0, 0, 0};
            double lo = (double)INFINITY;
            for (int i = 0; i < A * G; i++) {
                const size_t q = (size_t)b * A + (size_t)(i / G);
                const int g = i % G;
                if (g >= served[q]) continue;
                const size_t e = q * (size_t)G + (size_t)g;
                if (ep_i32[mpcx::RESPAWN_I32 * e + 7] != r) continue;
                mpcx::summary_take(ep_i32 + mpcx::RESPAWN_I32 * e, ep_f64 + mpcx::RESPAWN_F64 * e, acc, lo);
            }
            for (int k = 0; k < 4; k++) out_i64[4 * ((size_t)b * R + r) + k] = acc[k];
            out_f64[(size_t)b * R + r] = lo;
        }
}

// layout of mpcx_routes as the header's own compiler has it: sizeof, the offsets of its fields in order; then the sizes of the structs that
// routes travel beside and must not widen: mpcx_closed_loop, mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene, mpcx_admit,
// mpcx_respawn
extern "C" void route_ref_layout(int64_t *out17) {
    const size_t v[17] = {sizeof(mpcx_routes), offsetof(mpcx_routes, n_routes), offsetof(mpcx_routes, reserved), offsetof(mpcx_routes, route_off),
                          offsetof(mpcx_routes, route_len), offsetof(mpcx_routes, route_of), offsetof(mpcx_routes, start_state),
                          offsetof(mpcx_routes, start_idx), offsetof(mpcx_routes, path_off), offsetof(mpcx_routes, path_len),
                          sizeof(mpcx_closed_loop), sizeof(mpcx_closed_loop_opts), sizeof(mpcx_run_log), sizeof(mpcx_retire), sizeof(mpcx_scene),
                          sizeof(mpcx_admit), sizeof(mpcx_respawn)};
    for (int i = 0; i < 17; i++) out17[i] = (int64_t)v[i];
}

#ifdef ROUTE_REF_MAIN
// Runs the cases of a file written by tests/test_route_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_pool, u_len, G, has_log, has_prev_len, backwards, steps, R
//   the record of tests/respawn_ref/respawn_ref.cpp's main() --
//   f64: state (P,4), applied (P,2), u_sol (P,u_len), start_state (P,4), ep_f64 (P,G,2), min_clearance (P)
//   i32: traj_idx, target_ind, cut_len, iters, prev_len, own_row, done, steps_driven, wait, entered_step (P each), clock (1), start_idx (P),
//        due (P,G), served (P), ep_i32 (P,G,8), steps, goal_step, contact_step, flags (P each)
//   -- then the routes: i32 route_off (R), route_len (R), route_of (P,G), start_idx (P,G), path_off (P), path_len (P); f64 start_state (P,G,4)
// out per case and step: the mutable words -- state, applied, u_sol, ep_f64, min_clearance as f64, then traj_idx, target_ind, cut_len, iters,
// prev_len, steps_driven, wait, entered_step, served, ep_i32, steps, goal_step, contact_step, flags, path_off, path_len and the number arrived
// as int32.
template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T>
static void wr(FILE *g, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[9];
    while (fread(h, sizeof(int32_t), 9, f) == 9) {
        const size_t P = (size_t)h[0], G = (size_t)h[3], R = (size_t)h[8];
        const int n_pool = h[1], u_len = h[2], has_log = h[4], has_prev = h[5], backwards = h[6], steps = h[7];
        std::vector<double> state, applied, u, start_state, ep_f64, minc, rstate;
        std::vector<int32_t> traj, target, cut, iters, prev, own, done, driven, wait, entered, clock, start_idx, due, served, ep_i32, lsteps, goal,
            contact, flags, route_off, route_len, route_of, rstart, path_off, path_len;
        if (!rd(f, state, 4 * P) || !rd(f, applied, 2 * P) || !rd(f, u, (size_t)u_len * P) || !rd(f, start_state, 4 * P) || !rd(f, ep_f64, 2 * G * P) ||
            !rd(f, minc, P) || !rd(f, traj, P) || !rd(f, target, P) || !rd(f, cut, P) || !rd(f, iters, P) || !rd(f, prev, P) || !rd(f, own, P) ||
            !rd(f, done, P) || !rd(f, driven, P) || !rd(f, wait, P) || !rd(f, entered, P) || !rd(f, clock, 1) || !rd(f, start_idx, P) ||
            !rd(f, due, G * P) || !rd(f, served, P) || !rd(f, ep_i32, 8 * G * P) || !rd(f, lsteps, P) || !rd(f, goal, P) || !rd(f, contact, P) ||
            !rd(f, flags, P) || !rd(f, route_off, R) || !rd(f, route_len, R) || !rd(f, route_of, G * P) || !rd(f, rstart, G * P) ||
            !rd(f, path_off, P) || !rd(f, path_len, P) || !rd(f, rstate, 4 * G * P))
            return 5;
        mpcx_run_log log = {};
        log.steps = lsteps.data(); log.goal_step = goal.data(); log.contact_step = contact.data(); log.flags = flags.data();
        log.min_clearance = minc.data();
        mpcx_retire retire = {done.data(), driven.data(), 1.5, 0.1389};
        mpcx_admit admit = {wait.data(), entered.data(), clock.data(), 0, 0.0};
        mpcx_respawn rs = {(int32_t)G, 0, start_state.data(), start_idx.data(), due.data(), served.data(), ep_i32.data(), ep_f64.data()};
        mpcx_routes rt = {(int32_t)R, 0, route_off.data(), route_len.data(), route_of.data(), rstate.data(), rstart.data(), path_off.data(),
                          path_len.data()};
        for (int s = 0; s < steps; s++) {
            const int32_t got = route_ref_step((int)P, n_pool, u_len, state.data(), applied.data(), u.data(), traj.data(), target.data(), cut.data(),
                                               iters.data(), has_prev ? prev.data() : nullptr, own.data(), has_log ? &log : nullptr, &retire,
                                               &admit, &rs, &rt, backwards);
            wr(g, state); wr(g, applied); wr(g, u); wr(g, ep_f64); wr(g, minc);
            wr(g, traj); wr(g, target); wr(g, cut); wr(g, iters); wr(g, prev); wr(g, driven); wr(g, wait); wr(g, entered); wr(g, served);
            wr(g, ep_i32); wr(g, lsteps); wr(g, goal); wr(g, contact); wr(g, flags); wr(g, path_off); wr(g, path_len);
            fwrite(&got, sizeof(int32_t), 1, g);
            clock[0] += 1;          // the next step's admission stage would have advanced it
        }
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
