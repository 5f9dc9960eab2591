// Host build of csrc/mpcx_sight_core.h: the line-of-sight rule as a plain loop over host arrays.  The GPU's sight_kernel compiles the very
// same header.  Test infrastructure (tests/test_sight_cpu.py, tests/test_gpu_sight.py), also run under the sanitizers as a stand-alone
// program; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mpcx_sight_core.h"

// One step's stage for P agents, the arguments of the kernel with HOST pointers (done, absent and heard may be null).  backwards != 0: the
// agents are visited from the last to the first (the outcome must not depend on it).
extern "C" void sight_ref_step(int P, int n_pool, const double *state, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt,
                               const int32_t *obs_skip, const int32_t *done, const int32_t *absent, const double *hp, const int32_t *hp_off,
                               const double *box, const int32_t *set_off, const int32_t *set_of, const int32_t *heard, double range, int n_occ,
                               int n_sets, uint64_t *sight, int32_t *n_seen, int32_t *n_hidden, int backwards) {
    mpcx::SightArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.n_pool = n_pool;
    a.state = state; a.obs6 = obs6; a.obs_off = obs_off; a.obs_cnt = obs_cnt; a.obs_skip = obs_skip; a.done = done; a.absent = absent;
    a.s.sight = sight; a.s.n_seen = n_seen; a.s.n_hidden = n_hidden; a.s.hp = hp; a.s.hp_off = hp_off; a.s.box = box; a.s.set_off = set_off;
    a.s.set_of = set_of; a.s.heard = heard; a.s.range = range; a.s.n_occ = n_occ; a.s.n_sets = n_sets; a.s.n_rows = P; a.s.n_pool = n_pool;
    for (int k = 0; k < P; k++) mpcx::sight_agent(a, backwards ? P - 1 - k : k);
}

// layout of mpcx_sight as the header's own compiler has it: sizeof, then the offsets of its fifteen fields in order
extern "C" void sight_ref_layout(int64_t *out16) {
#define OFF(f) (int64_t)offsetof(mpcx_sight, f)
    const int64_t v[16] = {(int64_t)sizeof(mpcx_sight), OFF(sight), OFF(n_seen), OFF(n_hidden), OFF(hp), OFF(hp_off), OFF(box), OFF(set_off),
                           OFF(set_of), OFF(heard), OFF(range), OFF(n_occ), OFF(n_sets), OFF(n_rows), OFF(n_pool), OFF(reserved)};
#undef OFF
    for (int i = 0; i < 16; i++) out16[i] = v[i];
}

#ifdef SIGHT_REF_MAIN
// `sight_ref --layout` prints the sixteen numbers of sight_ref_layout.  `sight_ref in out` runs the cases of a file written by
// tests/sight_helpers.py and writes every case's words back.  Per case: int32 P, n_pool, n_occ, n_sets, hp_rows, has_done, has_absent,
// has_heard, backwards; double range; then int32 obs_off, obs_cnt, obs_skip, set_of (P each), done (P, if present), absent, heard (n_pool
// each, if present), hp_off (n_occ + 1), set_off (n_sets + 1); then double state (4 P), obs6 (6 n_pool), hp (3 hp_rows), box (4 n_occ).
// out per case: sight (P uint64), n_seen, n_hidden (P int32 each).
static bool rd(FILE *f, std::vector<int32_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(int32_t), n, f) == n; }
static bool rdd(FILE *f, std::vector<double> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(double), n, f) == n; }

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--layout")) {
        int64_t v[16];
        sight_ref_layout(v);
        for (int i = 0; i < 16; i++) printf("%lld%c", (long long)v[i], i == 15 ? '\n' : ' ');
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t h[9];
    while (fread(h, sizeof(int32_t), 9, f) == 9) {
        for (int i = 0; i < 5; i++) if (h[i] < 0) return 4;
        const size_t P = (size_t)h[0], np = (size_t)h[1], nocc = (size_t)h[2], nsets = (size_t)h[3], rows = (size_t)h[4];
        double range;
        if (fread(&range, sizeof(double), 1, f) != 1) return 4;
        std::vector<int32_t> off, cnt, skip, set_of, done, absent, heard, hp_off, set_off;
        if (!rd(f, off, P) || !rd(f, cnt, P) || !rd(f, skip, P) || !rd(f, set_of, P) || !rd(f, done, h[5] ? P : 0) || !rd(f, absent, h[6] ? np : 0) ||
            !rd(f, heard, h[7] ? np : 0) || !rd(f, hp_off, nocc + 1) || !rd(f, set_off, nsets + 1))
            return 5;
        std::vector<double> state, obs6, hp, box;
        if (!rdd(f, state, 4 * P) || !rdd(f, obs6, 6 * np) || !rdd(f, hp, 3 * rows) || !rdd(f, box, 4 * nocc)) return 6;
        std::vector<uint64_t> sight(P);
        std::vector<int32_t> seen(P), hidden(P);
        sight_ref_step((int)P, (int)np, state.data(), obs6.data(), off.data(), cnt.data(), skip.data(), h[5] ? done.data() : nullptr,
                       h[6] ? absent.data() : nullptr, hp.data(), hp_off.data(), box.data(), set_off.data(), set_of.data(),
                       h[7] ? heard.data() : nullptr, range, (int)nocc, (int)nsets, sight.data(), seen.data(), hidden.data(), h[8]);
        if (P) { fwrite(sight.data(), sizeof(uint64_t), P, g); fwrite(seen.data(), sizeof(int32_t), P, g); fwrite(hidden.data(), sizeof(int32_t), P, g); }
    }
    fclose(f); fclose(g);
    return 0;
}
#endif
