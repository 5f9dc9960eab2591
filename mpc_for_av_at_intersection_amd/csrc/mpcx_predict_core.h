// mpcx_predict_core.h -- the prediction of one pool row, shared by predict_kernel (mpcx_interaction_parts.h) and head_kernel (mpcx_prepare.hip):
// both evaluate these very expressions, in this spelling, so both leave the same bits.
#pragma once
#include "mpcx_common.h"

namespace mpcx {

// trajectories.py:11-37: the two disc centres (x, y, x, y) of a pose at (px, py) whose heading has cos / sin (c, s)
__device__ __forceinline__ void pose_discs(const mpcx_interaction_params &ip, double px, double py, double c, double s, double *out) {
#pragma unroll
    for (int d = 0; d < 2; d++) disc_centre(px, py, c, s, ip.circle_centers[2 * d], ip.circle_centers[2 * d + 1], out[2 * d], out[2 * d + 1]);
}

// moving_obstacles_prediction.py:21-28 for the pool row (x, y, v, yaw, acc, steer): v is updated BEFORE yaw; disc centres as
// trajectories.py:11-37.  out <- pred_steps frames of two disc centres; STAND: stand <- the two disc centres of the row's current pose
template <bool STAND>
__device__ __forceinline__ void predict_row(const mpcx_interaction_params &ip, double x, double y, double v, double yaw, double acc,
                                            double steer, double *stand, double *out) {
    const double tn = tan(steer);
    const double dt = ip.dt;
    double s, c;
    sincos(yaw, &s, &c);
    if constexpr (STAND) pose_discs(ip, x, y, c, s, stand);
    for (int k = 0; k < ip.pred_steps; k++) {
        x = __dadd_rn(x, __dmul_rn(__dmul_rn(v, c), dt));
        y = __dadd_rn(y, __dmul_rn(__dmul_rn(v, s), dt));
        v = __dadd_rn(v, __dmul_rn(acc, dt));
        yaw = __dadd_rn(yaw, __dmul_rn(__dmul_rn(__ddiv_rn(v, ip.L), tn), dt));
        sincos(yaw, &s, &c);
        pose_discs(ip, x, y, c, s, out + 4 * k);
    }
}

}  // namespace mpcx
