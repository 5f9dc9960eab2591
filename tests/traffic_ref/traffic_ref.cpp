// Host build of csrc/mpcx_traffic_core.h (the step rule of one scripted actor; the GPU's traffic_kernel compiles the very same header):
// test infrastructure that checks the rule against tapes recorded from the reference's classes and lets the sanitizers see it.
// Build with -ffp-contract=off (the rule's products are rounded one by one).  Never loaded by the product path.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mpcx_traffic_core.h"

// n_steps x (get(), step()) of one actor: rows[n_steps][6], state4 (x, y, theta, counter / cursor) in-out
extern "C" void traffic_ref_run(const mpcx_traffic_actor *a, double *state4, const double *tape, int64_t tape_rows, int n_steps, double *rows) {
    for (int k = 0; k < n_steps; k++) mpcx::traffic_get_step(*a, state4, tape, tape_rows, rows + 6 * k);
}
extern "C" int traffic_ref_actor_size(void) { return (int)sizeof(mpcx_traffic_actor); }
// layout of mpcx_closed_loop as the header has it: out[0] = sizeof, then the offsets of n_actors, pool_rows, actors, actor_state, tape,
// actor_row, ego_row, tape_rows, and of obs_local (the last field before the traffic block)
extern "C" void traffic_ref_closed_loop_layout(int64_t *out10) {
    const size_t v[10] = {sizeof(mpcx_closed_loop), offsetof(mpcx_closed_loop, n_actors), offsetof(mpcx_closed_loop, pool_rows),
                          offsetof(mpcx_closed_loop, actors), offsetof(mpcx_closed_loop, actor_state), offsetof(mpcx_closed_loop, tape),
                          offsetof(mpcx_closed_loop, actor_row), offsetof(mpcx_closed_loop, ego_row), offsetof(mpcx_closed_loop, tape_rows),
                          offsetof(mpcx_closed_loop, obs_local)};
    for (int i = 0; i < 10; i++) out10[i] = (int64_t)v[i];
}

#ifdef TRAFFIC_REF_MAIN
// in:  int32 n_cases, int32 n_steps, int64 tape_rows, tape[tape_rows][6], then per case (mpcx_traffic_actor, double state[4])
// out: per case rows[n_steps][6], state[4]
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t n = 0, steps = 0;
    int64_t tape_rows = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&steps, 4, 1, f) != 1 || fread(&tape_rows, 8, 1, f) != 1 || n < 0 || steps < 0 || tape_rows < 0) return 4;
    std::vector<double> tape((size_t)tape_rows * 6);
    if (tape_rows && fread(tape.data(), 48, (size_t)tape_rows, f) != (size_t)tape_rows) return 4;
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    std::vector<double> rows((size_t)steps * 6);
    for (int i = 0; i < n; i++) {
        mpcx_traffic_actor a;
        double st[4];
        if (fread(&a, sizeof a, 1, f) != 1 || fread(st, sizeof st, 1, f) != 1) return 4;
        traffic_ref_run(&a, st, tape.data(), tape_rows, steps, rows.data());
        fwrite(rows.data(), 48, (size_t)steps, g);
        fwrite(st, sizeof st, 1, g);
    }
    fclose(f);
    fclose(g);
    return 0;
}
#endif
