// Host build of csrc/mpcx_stopsign_core.h: the stop-sign rule as a plain loop over host arrays.  The GPU's stopsign_kernel compiles the
// very same header.  Test infrastructure (tests/test_stopsign_cpu.py, tests/test_gpu_stopsign.py); never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mpcx_stopsign_core.h"

// One step's stop-sign stage for the junctions of *ss (n_per agents each), the arguments of the kernel with HOST pointers (done may be
// null).  backwards != 0: the junctions are visited from the last to the first (the outcome must not depend on it).  Returns the agents
// waiting.
extern "C" int stopsign_ref_step(int P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                                 int32_t *cut_len, const int32_t *done, const mpcx_stopsign *ss, int backwards) {
    mpcx_signals sg;
    memset(&sg, 0, sizeof sg);
    sg.path_stop = ss->path_stop;
    const mpcx::StopSignArgs a{mpcx::SignalArgs{P, dl, state, path_off, path_len, traj_idx, cut_len, done, sg}, *ss};
    int got = 0;
    for (int k = 0; k < ss->n_junctions; k++) got += mpcx::stopsign_junction(a, backwards ? ss->n_junctions - 1 - k : k);
    return got;
}

// layout of mpcx_stopsign as the header's own compiler has it: sizeof, the offsets of its twenty-seven fields in order,
// MPCX_STOPSIGN_PER_MAX; then the sizes of the structs that the stage travels beside and must not widen: mpcx_closed_loop,
// mpcx_closed_loop_opts, mpcx_priority, mpcx_braking, mpcx_keepclear, mpcx_reservation, mpcx_signals
extern "C" void stopsign_ref_layout(int64_t *out36) {
#define OFF(f) (int64_t)offsetof(mpcx_stopsign, f)
    const int64_t v[36] = {(int64_t)sizeof(mpcx_stopsign), OFF(path_stop), OFF(path_move), OFF(path_exit), OFF(conflict), OFF(lane), OFF(sign),
                           OFF(gap), OFF(stopped_at), OFF(go), OFF(stopping), OFF(clock), OFF(ran), OFF(lag), OFF(blocker), OFF(occupied),
                           OFF(n_waiting), OFF(v_stop), OFF(brake), OFF(v_floor), OFF(zone), OFF(detect), OFF(patience), OFF(n_per),
                           OFF(n_junctions), OFF(n_moves), OFF(n_points), OFF(reserved), MPCX_STOPSIGN_PER_MAX,
                           (int64_t)sizeof(mpcx_closed_loop), (int64_t)sizeof(mpcx_closed_loop_opts), (int64_t)sizeof(mpcx_priority),
                           (int64_t)sizeof(mpcx_braking), (int64_t)sizeof(mpcx_keepclear), (int64_t)sizeof(mpcx_reservation),
                           (int64_t)sizeof(mpcx_signals)};
#undef OFF
    for (int i = 0; i < 36; i++) out36[i] = v[i];
}
