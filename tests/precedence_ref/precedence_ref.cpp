// Host build of csrc/mpcx_precedence_core.h: the entry-order stamp of MPCX_PRECEDENCE_ENTRY as a plain loop over host arrays.  The GPU's
// precedence_stamp_kernel compiles the very same header.  Test infrastructure (tests/test_precedence_cpu.py), also run under the sanitizers;
// never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_precedence_core.h"

// One step's stamp for P agents, the arguments of the kernel with HOST pointers.  backwards != 0: the lanes are visited from the last to the
// first (the outcome must not depend on it).  Returns the number of words written.
extern "C" int precedence_ref_stamp(int P, int n_rows, const int32_t *obs_off, const int32_t *own_row, const int32_t *entered_step,
                                    int32_t *prec, int backwards) {
    const mpcx::StampArgs a{P, n_rows, obs_off, own_row, entered_step, prec};
    int got = 0;
    for (int k = 0; k < P; k++) got += mpcx::precedence_stamp_agent(a, backwards ? P - 1 - k : k) ? 1 : 0;
    return got;
}

// layout of mpcx_precedence as the header's own compiler has it: sizeof, the offsets of its fields in order, the two mode values, the window
// and the last step whose word fits; then the sizes of the structs that precedence travels beside and must not widen: mpcx_closed_loop,
// mpcx_closed_loop_opts, mpcx_run_log, mpcx_retire, mpcx_scene, mpcx_admit, mpcx_respawn, mpcx_routes
extern "C" void precedence_ref_layout(int64_t *out17) {
    const int64_t v[17] = {(int64_t)sizeof(mpcx_precedence), (int64_t)offsetof(mpcx_precedence, prec), (int64_t)offsetof(mpcx_precedence, stand),
                           (int64_t)offsetof(mpcx_precedence, n_rows), (int64_t)offsetof(mpcx_precedence, mode), MPCX_PRECEDENCE_FIXED,
                           MPCX_PRECEDENCE_ENTRY, MPCX_PRECEDENCE_WINDOW, MPCX_PRECEDENCE_MAX_STEP,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_run_log),
                           (int64_t)sizeof(mpcx_retire), (int64_t)sizeof(mpcx_scene), (int64_t)sizeof(mpcx_admit), (int64_t)sizeof(mpcx_respawn),
                           (int64_t)sizeof(mpcx_routes)};
    for (int i = 0; i < 17; i++) out17[i] = v[i];
}

#ifdef PRECEDENCE_REF_MAIN
// Runs the cases of a file written by tests/test_precedence_cpu.py and writes every case's words back.  Per case:
//   int32 P, n_rows, backwards; then int32 obs_off (P), own_row (P), entered_step (P), prec (n_rows)
// out per case: prec (n_rows) and the number of words written, int32.
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[3];
    while (fread(h, sizeof(int32_t), 3, f) == 3) {
        const size_t P = (size_t)h[0], n_rows = (size_t)h[1];
        std::vector<int32_t> off, own, entered, prec;
        if (!rd(f, off, P) || !rd(f, own, P) || !rd(f, entered, P) || !rd(f, prec, n_rows)) return 5;
        const int32_t got = precedence_ref_stamp((int)P, (int)n_rows, off.data(), own.data(), entered.data(), prec.data(), h[2]);
        if (!prec.empty()) fwrite(prec.data(), sizeof(int32_t), prec.size(), g);
        fwrite(&got, sizeof(int32_t), 1, g);
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
