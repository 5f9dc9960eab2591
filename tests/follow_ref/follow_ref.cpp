// Host build of csrc/mpcx_follow_core.h: the car-following rule as a plain loop over host arrays.  The GPU's follow_kernel and
// follow_clamp_kernel compile the very same header.  Test infrastructure (tests/test_follow_cpu.py, tests/test_gpu_follow.py), also run
// under the sanitizers as a stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mpcx_follow_core.h"

static mpcx::FollowArgs make_args(int P, int W, int n_pool, int speed, double dl, int32_t *leader, double *gap, double *cap, const double *par6,
                                  int reach) {
    mpcx::FollowArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.W = W; a.n_pool = n_pool; a.speed = speed; a.dl = dl;
    a.fl.leader = leader; a.fl.gap = gap; a.fl.cap = cap;
    a.fl.standstill = par6[0]; a.fl.time_gap = par6[1]; a.fl.brake = par6[2]; a.fl.v_min = par6[3]; a.fl.lateral = par6[4]; a.fl.heading = par6[5];
    a.fl.reach = reach; a.fl.n_rows = P; a.fl.reserved = 0;
    return a;
}

// One step's search stage for P agents, the arguments of the kernel with HOST pointers (done, obs_skip and absent may be null).  par6:
// standstill, time_gap, brake, v_min, lateral, heading.  backwards != 0: the agents are visited from the last to the first (the outcome must
// not depend on it).  Writes leader, gap, cap (P each) and lowers cut_len; returns the number of agents with a leader.
extern "C" int follow_ref_step(int P, int n_pool, double dl, int speed, const double *state, const double *path_xyyaw, const int32_t *path_off,
                               const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len, const int32_t *done, const double *obs6,
                               const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip, const int32_t *absent, int32_t *leader,
                               double *gap, double *cap, const double *par6, int reach, int backwards) {
    mpcx::FollowArgs a = make_args(P, 0, n_pool, speed, dl, leader, gap, cap, par6, reach);
    a.state = state; a.path_xyyaw = path_xyyaw; a.path_off = path_off; a.path_len = path_len; a.traj_idx = traj_idx; a.cut_len = cut_len;
    a.done = done; a.obs6 = obs6; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip; a.absent = absent;
    int got = 0;
    for (int k = 0; k < P; k++) got += mpcx::follow_agent(a, backwards ? P - 1 - k : k) >= 0 ? 1 : 0;
    return got;
}

// One step's clamp for P agents with windows of W points: row 2 of xref (P x 4 x W) under cap (P)
extern "C" void follow_ref_clamp(int P, int W, const int32_t *done, double *cap, double *xref, int backwards) {
    const double none[6] = {0, 0, 0, 0, 0, 0};
    mpcx::FollowArgs a = make_args(P, W, 0, 1, 0.0, nullptr, nullptr, cap, none, 0);
    a.done = done; a.xref = xref;
    for (int k = 0; k < P; k++) mpcx::follow_clamp_agent(a, backwards ? P - 1 - k : k);
}

// layout of mpcx_following as the header's own compiler has it: sizeof, then the offsets of its twelve fields in order
extern "C" void follow_ref_layout(int64_t *out13) {
#define OFF(f) (int64_t)offsetof(mpcx_following, f)
    const int64_t v[13] = {(int64_t)sizeof(mpcx_following), OFF(leader), OFF(gap), OFF(cap), OFF(standstill), OFF(time_gap), OFF(brake), OFF(v_min),
                           OFF(lateral), OFF(heading), OFF(reach), OFF(n_rows), OFF(reserved)};
#undef OFF
    for (int i = 0; i < 13; i++) out13[i] = v[i];
}

#ifdef FOLLOW_REF_MAIN
// Runs the cases of a file written by tests/test_follow_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_pool, n_path, W, has_done, has_skip, has_absent, backwards, speed, reach; double dl, par6; then int32 path_off, path_len,
//   traj_idx, cut_len, obs_off, obs_cnt (P each), done, obs_skip (P each, if present), absent (n_pool, if present); then double state (4 P),
//   path (3 n_path), obs6 (6 n_pool), xref (4 P W)
// out per case: leader, cut_len (P int32 each), gap, cap (P doubles each), xref after the clamp (4 P W doubles), the number of leaders, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static bool rdd(FILE *f, std::vector<double> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(double), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[10];
    while (fread(h, sizeof(int32_t), 10, f) == 10) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], npath = (size_t)h[2], W = (size_t)h[3];
        double d[7];
        if (fread(d, sizeof(double), 7, f) != 7) return 4;
        std::vector<int32_t> off, len, ti, cut, ooff, ocnt, done, skip, absent;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, cut, P) || !rd(f, ooff, P) || !rd(f, ocnt, P) || !rd(f, done, h[4] ? P : 0) ||
            !rd(f, skip, h[5] ? P : 0) || !rd(f, absent, h[6] ? np : 0))
            return 5;
        std::vector<double> state, path, obs6, xref;
        if (!rdd(f, state, 4 * P) || !rdd(f, path, 3 * npath) || !rdd(f, obs6, 6 * np) || !rdd(f, xref, 4 * P * W)) return 6;
        std::vector<int32_t> leader(P);
        std::vector<double> gap(P), cap(P);
        const int32_t got = follow_ref_step((int)P, (int)np, d[0], h[8], state.data(), path.data(), off.data(), len.data(), ti.data(), cut.data(),
                                            h[4] ? done.data() : nullptr, obs6.data(), ooff.data(), ocnt.data(), h[5] ? skip.data() : nullptr,
                                            h[6] ? absent.data() : nullptr, leader.data(), gap.data(), cap.data(), d + 1, h[9], h[7]);
        follow_ref_clamp((int)P, (int)W, h[4] ? done.data() : nullptr, cap.data(), xref.data(), h[7]);
        if (P) {
            fwrite(leader.data(), sizeof(int32_t), P, g);
            fwrite(cut.data(), sizeof(int32_t), P, g);
            fwrite(gap.data(), sizeof(double), P, g);
            fwrite(cap.data(), sizeof(double), P, g);
            if (!xref.empty()) fwrite(xref.data(), sizeof(double), xref.size(), g);
        }
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
