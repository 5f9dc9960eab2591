// mpcx_interaction_sight.hip -- the line-of-sight kernels of the conflict search (mpcx_sight): interaction_sight_kernel<false> and <true>
// (the body of interaction_kernel<true, true, PREC> with SIGHT: the agent's word of seen rows is ANDed onto its ballot of present rows; with
// PREC the seen rows that yield are taken through their standing records).  The templates are mpcx_interaction_parts.h's; the
// instantiations are kept apart, here and nowhere else, as mpcx_interaction_prec.hip keeps those of precedence.
#include "mpcx_interaction_parts.h"

namespace mpcx {

void launch_interaction_sight(int P, size_t lds, hipStream_t st, const InterArgs &ia, const unsigned long long *sight, bool prec) {
    const InterSightArgs sa{ia, sight};
    if (prec) hipLaunchKernelGGL(interaction_sight_kernel<true>, dim3(P), dim3(64), lds, st, sa);
    else hipLaunchKernelGGL(interaction_sight_kernel<false>, dim3(P), dim3(64), lds, st, sa);
}

}  // namespace mpcx
