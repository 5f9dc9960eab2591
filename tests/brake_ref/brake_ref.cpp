// Host build of csrc/mpcx_brake_core.h: the firm-hold rule as a plain loop over host arrays.  The GPU's brake_mark_kernel and
// brake_clamp_kernel compile the very same header.  Test infrastructure (tests/test_brake_cpu.py, tests/test_gpu_brake.py), also run under
// the sanitizers as a stand-alone program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mpcx_brake_core.h"

static mpcx::BrakeArgs make_args(int P, int W, int speed, double dl, const int32_t *path_off, const int32_t *path_len, int32_t *traj_idx,
                                 const int32_t *done, const int32_t *path_stop, int n_points, int32_t *firm, int32_t *overran, double *brake_cap,
                                 double brake, double setback) {
    mpcx::BrakeArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.W = W; a.speed = speed; a.dl = dl;
    a.path_off = path_off; a.path_len = path_len; a.traj_idx = traj_idx; a.done = done; a.path_stop = path_stop; a.n_points = n_points;
    a.br.brake = brake; a.br.setback = setback; a.br.firm = firm; a.br.overran = overran; a.br.brake_cap = brake_cap;
    return a;
}

// One step's mark for P agents, the arguments of the kernel with HOST pointers (done, held, boxed, yielding may be null; target_ind and
// win_len too in cut mode).  backwards != 0: the agents are visited from the last to the first (the outcome must not depend on it).
// Returns the number of line-held agents.
extern "C" int brake_ref_mark(int P, double dl, int speed, const int32_t *path_off, const int32_t *path_len, int32_t *traj_idx, int32_t *target_ind,
                              int32_t *win_len, const int32_t *done, const int32_t *path_stop, int n_points, const int32_t *held,
                              const int32_t *boxed, const int32_t *yielding, int32_t *firm, int32_t *overran, double *brake_cap, double brake,
                              double setback, int backwards) {
    mpcx::BrakeArgs a = make_args(P, 0, speed, dl, path_off, path_len, traj_idx, done, path_stop, n_points, firm, overran, brake_cap, brake, setback);
    a.target_ind = target_ind; a.win_len = win_len; a.held = held; a.boxed = boxed; a.yielding = yielding;
    int got = 0;
    for (int k = 0; k < P; k++) got += mpcx::brake_mark_agent(a, backwards ? P - 1 - k : k) != 0 ? 1 : 0;
    return got;
}

// One step's clamp for P agents with windows of W points (len_seen and done may be null)
extern "C" void brake_ref_clamp(int P, int W, double dl, const double *state, const double *path_xyyaw, const int32_t *path_off,
                                const int32_t *path_len, int32_t *traj_idx, int32_t *len_seen, const int32_t *done, const int32_t *path_stop,
                                int n_points, int32_t *firm, int32_t *overran, double *brake_cap, double brake, double setback, double *xref,
                                int backwards) {
    mpcx::BrakeArgs a = make_args(P, W, 1, dl, path_off, path_len, traj_idx, done, path_stop, n_points, firm, overran, brake_cap, brake, setback);
    a.state = state; a.path_xyyaw = path_xyyaw; a.len_seen = len_seen; a.xref = xref;
    for (int k = 0; k < P; k++) mpcx::brake_clamp_agent(a, backwards ? P - 1 - k : k);
}

// layout of mpcx_braking as the header's own compiler has it: sizeof, then the offsets of its five fields in order
extern "C" void brake_ref_layout(int64_t *out6) {
#define OFF(f) (int64_t)offsetof(mpcx_braking, f)
    const int64_t v[6] = {(int64_t)sizeof(mpcx_braking), OFF(brake), OFF(setback), OFF(firm), OFF(overran), OFF(brake_cap)};
#undef OFF
    for (int i = 0; i < 6; i++) out6[i] = v[i];
}

#ifdef BRAKE_REF_MAIN
// Runs the cases of a file written by tests/test_brake_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_points, W, has_done, has_held, has_boxed, has_yielding, backwards, speed, has_len_seen; double dl, brake, setback; then int32
//   path_off, path_len, traj_idx, target_ind, overran (P each), done, held, boxed, yielding, len_seen (P each, if present), path_stop
//   (n_points); then double state (4 P), path (3 n_points), xref (4 P W)
// out per case: firm, win_len, target_ind, traj_idx, overran, len_seen (P int32 each; len_seen if present), brake_cap (P doubles), xref after
// the clamp (4 P W doubles), the number of line-held agents, int32.  The clamp runs in speed mode only.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static bool rdd(FILE *f, std::vector<double> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(double), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[10];
    while (fread(h, sizeof(int32_t), 10, f) == 10) {
        const size_t P = (size_t)h[0], np = (size_t)h[1], W = (size_t)h[2];
        double d[3];
        if (fread(d, sizeof(double), 3, f) != 3) return 4;
        std::vector<int32_t> off, len, ti, tgt, over, done, held, boxed, yld, seen, stop;
        if (!rd(f, off, P) || !rd(f, len, P) || !rd(f, ti, P) || !rd(f, tgt, P) || !rd(f, over, P) || !rd(f, done, h[3] ? P : 0) ||
            !rd(f, held, h[4] ? P : 0) || !rd(f, boxed, h[5] ? P : 0) || !rd(f, yld, h[6] ? P : 0) || !rd(f, seen, h[9] ? P : 0) || !rd(f, stop, np))
            return 5;
        std::vector<double> state, path, xref;
        if (!rdd(f, state, 4 * P) || !rdd(f, path, 3 * np) || !rdd(f, xref, 4 * P * W)) return 6;
        std::vector<int32_t> firm(P), win(P);
        std::vector<double> cap(P);
        const int32_t got = brake_ref_mark((int)P, d[0], h[8], off.data(), len.data(), ti.data(), tgt.data(), win.data(), h[3] ? done.data() : nullptr,
                                           stop.data(), (int)np, h[4] ? held.data() : nullptr, h[5] ? boxed.data() : nullptr,
                                           h[6] ? yld.data() : nullptr, firm.data(), over.data(), cap.data(), d[1], d[2], h[7]);
        if (h[8])
            brake_ref_clamp((int)P, (int)W, d[0], state.data(), path.data(), off.data(), len.data(), ti.data(), h[9] ? seen.data() : nullptr,
                            h[3] ? done.data() : nullptr, stop.data(), (int)np, firm.data(), over.data(), cap.data(), d[1], d[2], xref.data(), h[7]);
        if (P) {
            fwrite(firm.data(), sizeof(int32_t), P, g);
            fwrite(win.data(), sizeof(int32_t), P, g);
            fwrite(tgt.data(), sizeof(int32_t), P, g);
            fwrite(ti.data(), sizeof(int32_t), P, g);
            fwrite(over.data(), sizeof(int32_t), P, g);
            if (h[9]) fwrite(seen.data(), sizeof(int32_t), P, g);
            fwrite(cap.data(), sizeof(double), P, g);
            if (!xref.empty()) fwrite(xref.data(), sizeof(double), xref.size(), g);
        }
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
