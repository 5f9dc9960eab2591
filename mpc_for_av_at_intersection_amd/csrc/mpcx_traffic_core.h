// mpcx_traffic_core.h -- the step rule of ONE scripted actor, host + device source (the pattern of mpcx_qp_stage.h): a restatement of
// this package's lib/moving_obstacles.py (reference: main/lib/moving_obstacles.py:16-231, plant main/bicycle/main.py:28-41).
// traffic_kernel (mpcx_traffic.hip) runs it one lane per actor; tests/traffic_ref/traffic_ref.cpp builds it for the host.
//
//   traffic_get_step(actor, state, tape, tape_rows, row)   row <- get(): (x, y, v, yaw, a = 0, steer); then step()
//
// The quirks are the classes' own:
//   - start delay: standing (v = 0) until counter > offset / counter_dt; offset <= 0 means no delay at all.  The roundabout class
//     counts with 0.2 s whatever the plant's sample time is -- the host puts that into counter_dt;
//   - get() reads (x, y, v, theta) and THEN the steering angle, and reading the roundabout's steering angle may snap the heading to
//     -pi / 0 once the vehicle has come around: the row carries the heading from before the snap, step() starts from the snapped one
//     (and reads the steering angle again: same answer, the conditions look at x and y only);
//   - T-intersection: a turning vehicle steers -0.38 (from the left) / +0.19 (from the right) from x_turn on until the heading has swept
//     a quarter turn (theta > -pi/2, theta < 3 pi/2);
//   - the plant integrates (v cos, v sin, (v / L) tan(delta)) * dt, each product rounded on its own.  NO FMA CONTRACTION, in any build:
//     every function below switches contraction off for its own statements (#pragma clang fp contract(off); a g++ host build passes -ffp-contract=off instead)
//     and spells the arithmetic as plain * + /, so neither hipcc's default -ffp-contract=fast nor a host -ffp-contract flag can fuse
//     x + dx * dt.  (The __dmul_rn / __dadd_rn of HIP's math header are plain operators inside ITS functions and fuse after inlining;
//     tests/test_traffic_cpu.py compiles the kernel with and without -ffp-contract=off and wants the same instructions.)
// The decisions compare values that are exact copies or sums of the above, so with the same libm the poses are the classes' bit for
// bit, and with another libm (the device's sin / cos / tan) only the poses move, by that libm's last bits -- a vehicle whose heading
// stays 0 (cos = 1, sin = 0, tan(0) = 0 in every libm) is bit-identical on the device too.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mpcx.h"

#if defined(__HIPCC__)
#define MPCX_TR_FN __host__ __device__ __forceinline__
#else
#define MPCX_TR_FN static inline
#endif
#if defined(__clang__)
#define MPCX_TR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else       /* g++ honours no such pragma: a host build with it passes -ffp-contract=off (tests/test_traffic_cpu.py) */
#define MPCX_TR_NO_CONTRACT
#endif

namespace mpcx {

constexpr double TR_PI = 3.141592653589793;      // numpy.pi

// _ScriptedVehicle.forward_velocity
MPCX_TR_FN double traffic_velocity(const mpcx_traffic_actor &a, double counter) {
    MPCX_TR_NO_CONTRACT
    const bool waiting = a.offset > 0.0 && !(counter > a.offset / a.counter_dt);
    return waiting ? 0.0 : a.speed;
}

// the `steering_angle` property of the three classes; may write theta (roundabout)
MPCX_TR_FN double traffic_steering(const mpcx_traffic_actor &a, double x, double y, double &theta) {
    if (a.kind == MPCX_TRAFFIC_ARTERIAL || !a.turning) return 0.0;
    if (a.kind == MPCX_TRAFFIC_TINTERSECTION) {
        if (a.direction == 1) return (x >= a.x_turn && theta > -TR_PI / 2.0) ? -0.38 : 0.0;
        return (x <= a.x_turn && theta < (3.0 * TR_PI) / 2.0) ? 0.19 : 0.0;
    }
    double delta = 0.0;     // MPCX_TRAFFIC_ROUNDABOUT: position-triggered arcs of radius 5 around the island
    if (a.direction == 1) {
        if (-7.0 <= x && x <= -4.0 && y < 0.0) delta = -a.arc;
        if (-3.0 < x) delta = a.arc;
        if (y > 0.0 && -5.0 <= x && x <= -3.0) delta = -a.arc;
        if (x <= -3.0 && y > 0.0) { theta = -TR_PI; delta = 0.0; }
    } else {
        if (4.0 <= x && x <= 7.0 && y > 0.0) delta = -a.arc;
        if (x < 3.0) delta = a.arc;
        if (y < 0.0 && 3.0 <= x && x <= 5.0) delta = -a.arc;
        if (3.0 <= x && y < 0.0) { theta = 0.0; delta = 0.0; }
    }
    return delta;
}

// get() into row[6], then step() on st[4] = (x, y, theta, counter).  tape: the uploaded table (TAPE actors only), tape_rows its length.
MPCX_TR_FN void traffic_get_step(const mpcx_traffic_actor &a, double *st, const double *tape, int64_t tape_rows, double *row) {
    MPCX_TR_NO_CONTRACT
    if (a.kind == MPCX_TRAFFIC_TAPE) {
        // cursor advances by one per step and stays on the actor's last row; the index is clamped into the table whatever the actor says
        const int64_t n = a.tape_rows > 0 ? a.tape_rows : 1;
        int64_t cur = (int64_t)st[3];
        if (cur < 0) cur = 0;
        if (cur > n - 1) cur = n - 1;
        int64_t r = (int64_t)a.tape_off + cur * (int64_t)a.tape_stride;
        if (r < 0) r = 0;
        if (r > tape_rows - 1) r = tape_rows - 1;
        for (int k = 0; k < 6; k++) row[k] = tape_rows > 0 ? tape[6 * r + k] : 0.0;      // (tape_rows = 0: no table)
        st[0] = row[0]; st[1] = row[1]; st[2] = row[3];
        st[3] = (double)(cur < n - 1 ? cur + 1 : cur);
        return;
    }
    double x = st[0], y = st[1], theta = st[2];
    const double counter = st[3];
    const double v = traffic_velocity(a, counter);
    row[0] = x; row[1] = y; row[2] = v; row[3] = theta; row[4] = 0.0;
    row[5] = traffic_steering(a, x, y, theta);                 // get(): the heading in the row is the one from before a snap
    const double delta = traffic_steering(a, x, y, theta);     // step(): reads it again
    const double c = cos(theta), s = sin(theta);
    const double dx = v * c, dy = v * s;
    const double dth = (v / a.L) * tan(delta);
    st[0] = x + dx * a.model_dt;
    st[1] = y + dy * a.model_dt;
    st[2] = theta + dth * a.model_dt;
    st[3] = counter + 1.0;
}

}  // namespace mpcx
