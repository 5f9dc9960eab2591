// Host build of csrc/mpcx_safety_core.h: the near-miss rule and the conflict matrix as plain loops over host arrays.  The GPU's
// safety_kernel and safety_summary_kernel compile the very same header.  Test infrastructure (tests/test_safety_cpu.py,
// tests/test_gpu_safety.py), also run under the sanitizers as a stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mpcx_safety_core.h"

// One step's stage for P agents, the arguments of the kernel with HOST pointers (done and absent may be null).  geo5: radius and the four
// circle_centers.  words7: partner, ttc_row, ttc_frame, tick, enc_row, n_events (P int32 each) and ev_i32 (P x capacity x 8).  backwards
// != 0: the agents are visited from the last to the first (the outcome must not depend on it).
extern "C" void safety_ref_step(int P, int n_pool, int pred_steps, const double *geo5, const double *obs6, const double *pred, const double *state,
                                const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip, const int32_t *traj_idx,
                                const int32_t *path_off, const int32_t *done, const int32_t *absent, const int32_t *row_agent, int32_t *partner,
                                double *clearance, int32_t *ttc_row, int32_t *ttc_frame, int32_t *tick, int32_t *enc_row, int32_t *n_events,
                                int32_t *ev_i32, double *ev_f64, double near, int ttc_frames, int capacity, int backwards) {
    mpcx::SafetyArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.n_pool = n_pool; a.pred_steps = pred_steps; a.radius = geo5[0];
    for (int i = 0; i < 4; i++) a.cc[i] = geo5[1 + i];
    a.obs6 = obs6; a.pred = pred; a.state = state; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip; a.traj_idx = traj_idx;
    a.path_off = path_off; a.done = done; a.absent = absent;
    a.s.partner = partner; a.s.clearance = clearance; a.s.ttc_row = ttc_row; a.s.ttc_frame = ttc_frame; a.s.tick = tick; a.s.enc_row = enc_row;
    a.s.n_events = n_events; a.s.ev_i32 = ev_i32; a.s.ev_f64 = ev_f64; a.s.row_agent = row_agent;
    a.s.near = near; a.s.ttc_frames = ttc_frames; a.s.capacity = capacity; a.s.n_rows = P; a.s.n_pool = n_pool;
    for (int k = 0; k < P; k++) mpcx::safety_agent(a, backwards ? P - 1 - k : k);
}

// The conflict matrix of P / A instances: out_i64 (B, R + 1, R + 1, 3), out_f64 (B, R + 1, R + 1, 2)
extern "C" void safety_ref_summary(int P, int A, int capacity, int R, const int32_t *route_off, double dt, const int32_t *n_events,
                                   const int32_t *ev_i32, const double *ev_f64, int64_t *out_i64, double *out_f64) {
    const int C = R + 1;
    for (int b = 0; b < P / A; b++)
        for (int ci = 0; ci < C; ci++)
            for (int cj = 0; cj < C; cj++) {
                int64_t acc[mpcx::SAFETY_SUM_I64] = {0, 0, 0};
                double lo = INFINITY;
                int32_t kmin = INT32_MAX;
                for (int q = b * A; q < (b + 1) * A; q++)
                    for (int e = 0; e < capacity && e < n_events[q]; e++) {
                        const size_t at = (size_t)q * capacity + e;
                        const int32_t *w = ev_i32 + mpcx::SAFETY_I32 * at;
                        if (mpcx::safety_class(route_off, R, w[4]) != ci || mpcx::safety_class(route_off, R, w[5]) != cj) continue;
                        mpcx::safety_take(w, ev_f64 + mpcx::SAFETY_F64 * at, acc, lo, kmin);
                    }
                const size_t cell = ((size_t)b * C + ci) * C + cj;
                for (int k = 0; k < mpcx::SAFETY_SUM_I64; k++) out_i64[mpcx::SAFETY_SUM_I64 * cell + k] = acc[k];
                out_f64[mpcx::SAFETY_SUM_F64 * cell] = lo;
                out_f64[mpcx::SAFETY_SUM_F64 * cell + 1] = mpcx::safety_seconds(kmin, dt);
            }
}

// layout of mpcx_safety as the header's own compiler has it: sizeof, then the offsets of its sixteen fields in order
extern "C" void safety_ref_layout(int64_t *out17) {
#define OFF(f) (int64_t)offsetof(mpcx_safety, f)
    const int64_t v[17] = {(int64_t)sizeof(mpcx_safety), OFF(partner), OFF(clearance), OFF(ttc_row), OFF(ttc_frame), OFF(tick), OFF(enc_row),
                           OFF(n_events), OFF(ev_i32), OFF(ev_f64), OFF(row_agent), OFF(near), OFF(ttc_frames), OFF(capacity), OFF(n_rows),
                           OFF(n_pool), OFF(reserved)};
#undef OFF
    for (int i = 0; i < 17; i++) out17[i] = v[i];
}

#ifdef SAFETY_REF_MAIN
// Runs the cases of a file written by tests/test_safety_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_pool, pred_steps, has_done, has_absent, backwards, ttc_frames, capacity, n_steps, A, R; double near, dt, geo5; then int32
//   obs_off, obs_cnt, obs_skip, traj_idx, path_off (P each), done (P, if present), absent (n_pool, if present), row_agent (n_pool), tick,
//   enc_row, n_events (P each), ev_i32 (8 P capacity), route_off (R); then double state (4 P), ev_f64 (2 P capacity), and per step obs6
//   (6 n_pool) and pred (4 pred_steps n_pool).
// The stage runs n_steps times, each on its own obs6 and pred.  out per case: per step partner, ttc_row, ttc_frame (P int32 each) and
// clearance (P doubles); then tick, enc_row, n_events, ev_i32, ev_f64; then the conflict matrix of instances of A agents over R routes.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static bool rdd(FILE *f, std::vector<double> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(double), n, f) == n; }
static void wr(FILE *g, const std::vector<int32_t> &v) { if (!v.empty()) fwrite(v.data(), sizeof(int32_t), v.size(), g); }
static void wrd(FILE *g, const std::vector<double> &v) { if (!v.empty()) fwrite(v.data(), sizeof(double), v.size(), g); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[11];
    while (fread(h, sizeof(int32_t), 11, f) == 11) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], S = (size_t)h[2], cap = (size_t)h[7], R = (size_t)h[10];
        const int A = h[9];
        double d[7];
        if (fread(d, sizeof(double), 7, f) != 7) return 4;
        std::vector<int32_t> off, cnt, skip, ti, poff, done, absent, owner, tick, enc, nev, ev, routes;
        if (!rd(f, off, P) || !rd(f, cnt, P) || !rd(f, skip, P) || !rd(f, ti, P) || !rd(f, poff, P) || !rd(f, done, h[3] ? P : 0) ||
            !rd(f, absent, h[4] ? np : 0) || !rd(f, owner, np) || !rd(f, tick, P) || !rd(f, enc, P) || !rd(f, nev, P) || !rd(f, ev, 8 * P * cap) ||
            !rd(f, routes, R))
            return 5;
        std::vector<double> state, evf, obs6, pred;
        if (!rdd(f, state, 4 * P) || !rdd(f, evf, 2 * P * cap)) return 6;
        std::vector<int32_t> partner(P), trow(P), tframe(P);
        std::vector<double> clr(P);
        for (int s = 0; s < h[8]; s++) {
            if (!rdd(f, obs6, 6 * np) || !rdd(f, pred, 4 * S * np)) return 7;
            safety_ref_step((int)P, (int)np, (int)S, d + 2, obs6.data(), pred.data(), state.data(), off.data(), cnt.data(), skip.data(), ti.data(),
                            poff.data(), h[3] ? done.data() : nullptr, h[4] ? absent.data() : nullptr, owner.data(), partner.data(), clr.data(),
                            trow.data(), tframe.data(), tick.data(), enc.data(), nev.data(), ev.data(), evf.data(), d[0], h[6], (int)cap, h[5]);
            wr(g, partner); wr(g, trow); wr(g, tframe); wrd(g, clr);
        }
        wr(g, tick); wr(g, enc); wr(g, nev); wr(g, ev); wrd(g, evf);
        if (A > 0 && P % (size_t)A == 0) {
            const size_t cells = P / (size_t)A * (R + 1) * (R + 1);
            std::vector<int64_t> oi(3 * cells);
            std::vector<double> of(2 * cells);
            safety_ref_summary((int)P, A, (int)cap, (int)R, routes.data(), d[1], nev.data(), ev.data(), evf.data(), oi.data(), of.data());
            if (cells) { fwrite(oi.data(), sizeof(int64_t), oi.size(), g); fwrite(of.data(), sizeof(double), of.size(), g); }
        }
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
