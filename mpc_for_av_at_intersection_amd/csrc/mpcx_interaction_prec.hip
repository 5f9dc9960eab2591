// mpcx_interaction_prec.hip -- the right-of-way instantiations of the conflict search's kernels (mpcx_precedence): predict_kernel<·, true, true>
// (STAND: every predicted row also leaves its standing record) and interaction_kernel<true, true, true> (PREC: the present rows that yield to
// the agent are seen through their standing records).  The templates are mpcx_interaction_parts.h's; the instantiations are kept apart, here
// and nowhere else, so that mpcx_interaction.hip holds exactly the kernels it held before there was precedence.
#include "mpcx_interaction_parts.h"

namespace mpcx {

void launch_predict_stand(bool mapped, int lanes, hipStream_t st, const PredArgs &pa) {
    if (mapped) hipLaunchKernelGGL((predict_kernel<true, true, true>), dim3((lanes + 63) / 64), dim3(64), 0, st, pa);
    else hipLaunchKernelGGL((predict_kernel<false, true, true>), dim3((lanes + 63) / 64), dim3(64), 0, st, pa);
}

void launch_interaction_prec(int P, size_t lds, hipStream_t st, const InterArgs &ia) {
    hipLaunchKernelGGL((interaction_kernel<true, true, true>), dim3(P), dim3(64), lds, st, ia);
}

}  // namespace mpcx
