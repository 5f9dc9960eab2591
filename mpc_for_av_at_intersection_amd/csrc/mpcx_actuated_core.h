// mpcx_actuated_core.h -- VEHICLE-ACTUATED SIGNALS: a controller per junction decides the lights from who is waiting in front of the stop
// lines.  Host + device source (the pattern of mpcx_signal_core.h, whose hold it shares).  actuated_signal_kernel (mpcx_actuated.hip) runs
// it with a lane group per junction in the place of signal_kernel; tests/actuated_ref/actuated_ref.cpp builds it for the host.
//
// A junction is n_per consecutive agents: junction j owns agents [j n_per, (j + 1) n_per).  A controller has n_phases phases (1..8):
// phase_groups[c][k] the bitmask of the signal groups green in phase k, phase_time[c][k] = (min_green, max_green, gap) in steps,
// ctrl_time[c] = (amber, all_red in steps, detect in path points); ctrl_of[j] the controller of junction j.  jstate[j] = (phase, stage,
// timer, idle), stage 0 GREEN, 1 AMBER, 2 ALL_RED; lights[j] 2 bits per group (MPCX_SIGNAL_*); calls[j] bit g = group g is called.
// Integers only.
//
// Per junction and step, in this order:
//   1. read (p, stage, timer, idle); a defective word (p outside [0, n_phases), stage outside 0..2, timer < 0 or idle < 0) counts as
//      (0, GREEN, 0, 0).  ctrl_of[j] out of range: no controller -- the agents are free (held = 0), jstate is left alone, lights = calls = 0.
//   2. the lights of this step from the state as read: GREEN -- the groups of phase_groups[p] green, all others red; AMBER -- those groups
//      amber, all others red; ALL_RED -- all red.
//   3. calls: bit g is set if some agent q of the junction is not done, stands on a valid point in front of its line (the validity tests
//      of the signal rule's step 3) with group g, and is inside the detector: s - traj_idx[q] <= detect.
//   4. advance, with D_k = (calls & phase_groups[k]) != 0 and other = some k != p has D_k.  GREEN: timer' = min(timer + 1, max_green),
//      idle' = D_p ? 0 : min(idle + 1, gap); leave if other && timer' >= min_green && (idle' >= gap || timer' >= max_green), else rest in
//      green.  AMBER: timer' = timer + 1, leave at timer' >= amber; ALL_RED the same with all_red.  Leaving goes GREEN -> AMBER -> ALL_RED
//      -> GREEN of the next phase, timer = idle = 0 on entry; a stage of length 0 is passed through in the same step.  The next phase is
//      the first k in ring order p + 1, p + 2, ... (mod n_phases, p excluded) with D_k, (p + 1) % n_phases if there is none.
//   5. every agent of the junction: signal_hold (mpcx_signal_core.h) with the light of its group from lights[j].
// A junction's words are read before any of them is written, its agents' words are the agents' own: the outcome does not depend on the
// order of the junctions, nor on that of the agents of a junction.
#pragma once
#include "mpcx_signal_core.h"

namespace mpcx {

struct ActuatedArgs {
    SignalArgs s;           // the hold's words: s.sg supplies path_stop, path_group, held, brake, n_points, n_groups
    mpcx_actuation ac;
};

struct JunctionWord {
    int32_t phase, stage, timer, idle;
};

// the controller of junction j, -1 = none
MPCX_REC_FN int32_t actuated_ctrl(const mpcx_actuation &c, int j) {
    const int32_t k = c.ctrl_of[j];
    return k >= 0 && k < c.n_ctrl ? k : -1;
}

// step 1: the state as read
MPCX_REC_FN JunctionWord actuated_read(const mpcx_actuation &c, int j) {
    const int32_t *w = c.jstate + 4 * (size_t)j;
    JunctionWord s{w[0], w[1], w[2], w[3]};
    if (s.phase < 0 || s.phase >= c.n_phases || s.stage < MPCX_STAGE_GREEN || s.stage > MPCX_STAGE_ALL_RED || s.timer < 0 || s.idle < 0)
        s = JunctionWord{0, MPCX_STAGE_GREEN, 0, 0};
    return s;
}

// step 2: the light word of a state whose phase has the group mask `mask`
MPCX_REC_FN uint32_t actuated_lights(uint32_t mask, int32_t stage, int32_t n_groups) {
    uint32_t w = 0;
    for (int g = 0; g < n_groups; g++) {
        const bool on = stage != MPCX_STAGE_ALL_RED && ((mask >> g) & 1u) != 0;
        const uint32_t code = on ? (stage == MPCX_STAGE_GREEN ? MPCX_SIGNAL_GREEN : MPCX_SIGNAL_AMBER) : MPCX_SIGNAL_RED;
        w |= code << (2 * g);
    }
    return w;
}

// step 3 for one agent: its call bit, 0 = it does not call
MPCX_REC_FN uint32_t actuated_call(const SignalArgs &a, int q, int32_t detect) {
    const mpcx_signals &g = a.sg;
    if (a.done && a.done[q] != 0) return 0;
    const int32_t ti = a.traj_idx[q];
    const int64_t i = (int64_t)a.path_off[q] + (int64_t)ti;
    if (i < 0 || i >= (int64_t)g.n_points) return 0;
    const int32_t s = g.path_stop[i], grp = g.path_group[i];
    if (s < 0 || s >= a.path_len[q] || ti >= s || grp < 0 || grp >= g.n_groups) return 0;
    return (int64_t)s - (int64_t)ti <= (int64_t)detect ? 1u << grp : 0u;
}

// step 4: the state of the next step under controller k and this step's calls
MPCX_REC_FN JunctionWord actuated_advance(const mpcx_actuation &c, int32_t k, JunctionWord s, uint32_t calls) {
    const int32_t n = c.n_phases;
    const int32_t *masks = c.phase_groups + (size_t)k * (size_t)n;
    const int32_t *pt = c.phase_time + 3 * ((size_t)k * (size_t)n + (size_t)s.phase);
    const int32_t amber = c.ctrl_time[3 * (size_t)k], all_red = c.ctrl_time[3 * (size_t)k + 1];
    int32_t next = s.phase + 1 < n ? s.phase + 1 : 0;
    bool other = false;
    for (int d = 1; d < n; d++) {
        const int32_t kk = s.phase + d < n ? s.phase + d : s.phase + d - n;
        if ((calls & (uint32_t)masks[kk]) != 0) { other = true; next = kk; break; }
    }
    bool leave;
    if (s.stage == MPCX_STAGE_GREEN) {
        const int32_t min_green = pt[0], max_green = pt[1], gap = pt[2];
        const bool own = (calls & (uint32_t)masks[s.phase]) != 0;
        s.timer = s.timer < max_green ? s.timer + 1 : max_green;
        s.idle = own ? 0 : s.idle < gap ? s.idle + 1 : gap;
        leave = other && s.timer >= min_green && (s.idle >= gap || s.timer >= max_green);
        if (leave) s = JunctionWord{s.phase, MPCX_STAGE_AMBER, 0, 0};
    } else {
        const int32_t len = s.stage == MPCX_STAGE_AMBER ? amber : all_red;
        leave = (int64_t)s.timer + 1 >= (int64_t)len;
        if (leave) s = JunctionWord{s.phase, s.stage + 1, 0, 0};
        else s.timer += 1;
    }
    if (leave) {        // entered a stage with timer 0: a stage of length 0 is passed through in the same step
        if (s.stage == MPCX_STAGE_AMBER && amber <= 0) s.stage = MPCX_STAGE_ALL_RED;
        if (s.stage == MPCX_STAGE_ALL_RED && all_red <= 0) s.stage = MPCX_STAGE_ALL_RED + 1;
        if (s.stage > MPCX_STAGE_ALL_RED) s = JunctionWord{next, MPCX_STAGE_GREEN, 0, 0};
    }
    return s;
}

// the light of a group from a junction's light word
struct WordLight {
    uint32_t lights;
    MPCX_REC_FN_MEMBER int operator()(int32_t grp) const { return (int)((lights >> (2 * grp)) & 3u); }
};

// the whole rule for junction j as one loop (the host's order; the kernel spreads the agents over a lane group); returns the agents held
MPCX_REC_FN int actuated_junction(const ActuatedArgs &a, int j) {
    const mpcx_actuation &c = a.ac;
    const int q0 = j * c.n_per;
    const int32_t k = actuated_ctrl(c, j);
    uint32_t lights = 0, calls = 0;
    if (k >= 0) {
        const JunctionWord s = actuated_read(c, j);
        lights = actuated_lights((uint32_t)c.phase_groups[(size_t)k * (size_t)c.n_phases + (size_t)s.phase], s.stage, a.s.sg.n_groups);
        const int32_t detect = c.ctrl_time[3 * (size_t)k + 2];
        for (int q = q0; q < q0 + c.n_per; q++) calls |= actuated_call(a.s, q, detect);
        const JunctionWord t = actuated_advance(c, k, s, calls);
        int32_t *w = c.jstate + 4 * (size_t)j;
        w[0] = t.phase; w[1] = t.stage; w[2] = t.timer; w[3] = t.idle;
    }
    c.lights[j] = (int32_t)lights;
    c.calls[j] = (int32_t)calls;
    int got = 0;
    for (int q = q0; q < q0 + c.n_per; q++) got += signal_hold(a.s, q, k >= 0, WordLight{lights}) != 0 ? 1 : 0;
    return got;
}

}  // namespace mpcx
