// mpcx_loop.hip -- the reference's scenario loop body (main/scenarios/mpc_intersection.py:95-159) for P agents as a
// device-resident pipeline (and, with MPCX_STOP_SPEED, that of main/scenarios/mpc_intersection_new_ref.py:90-159: the same stages, the
// path kept whole and the speed reference zeroed from the conflict on):
// n_steps x [scripted traffic rows -> pool pack -> predict -> conflict search + path cut -> reference window ->
// rollout -> QP -> plant (-> run-log record, iff a log is attached)], enqueued back to back on the context's stream (optionally as a replayed hipGraph), no
// host synchronisation or host arithmetic in between.  With retirement at the goal (mpcx_retire) the step ends with retire_kernel, and an agent
// that has arrived is skipped by every stage but the pool pack; with a scene (mpcx_scene) its arrival also takes it out of everybody
// else's obstacle list; with admission (mpcx_admit) the step begins with the two launches that let waiting agents in; with respawn
// (mpcx_respawn) it ends with respawn_kernel, which resets an arrived agent's slot for the next vehicle of its stream; with right of way
// (mpcx_precedence) the conflict search shows an agent the cars that yield to it as standing cars; with traffic signals (mpcx_signals) one
// more launch behind the conflict search holds agents at their stop lines (mpcx_actuation: its lights follow the demand).
// Every stage is the kernel behind the per-stage C entry
// point, called with the very buffers the descriptor names, so a run is bit-identical to driving the stages one
// by one from the host.  With step fusion (mpcx_set_step_fusion, enqueue_fused_run) a run without any of the optional stages takes the plant
// update of the step before, the pool pack, the prediction and the rollout in one launch per step: the same bits in every buffer.
#include "mpcx_common.h"
#include <cmath>
#include <cstring>

namespace mpcx {

struct PackArgs {
    int P;
    const double *state, *applied;
    double *obs6;
};

// MovingObstacle*.get() of the reference (mpc_intersection.py:119-122): (x, y, v, yaw, a, steer)
__global__ __launch_bounds__(256) void pack_pool_kernel(PackArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.P) return;
    double *o = a.obs6 + 6 * (size_t)q;
    const double *s = a.state + 4 * (size_t)q;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
    o[4] = a.applied[2 * q + 1];
    o[5] = a.applied[2 * q];
}

}  // namespace mpcx

// the agents' pool rows (device) lie inside the pool; who: what the message starts with
static int32_t mpcx_loop_check_rows(mpcx_ctx *ctx, int32_t P, const int32_t *ego_row, int32_t pool_rows, const char *who = "closed_loop_run") {
    std::vector<int32_t> rows((size_t)P);
    if (hipMemcpy(rows.data(), ego_row, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return mpcx_fail(ctx, MPCX_E_LAUNCH, "%s: cannot read the agents' pool rows back for their check", who);
    for (int32_t q = 0; q < P; q++)
        if (rows[q] < 0 || rows[q] >= pool_rows)
            return mpcx_fail(ctx, MPCX_E_INVALID, "%s: agent %d sits in pool row %d of %d", who, q, rows[q], pool_rows);
    return MPCX_OK;
}

// the second part of ctx->prev_cut: 3 ints per agent that the conflict search leaves for the window selection (mpcx_interaction_extras::near)
static int32_t *near_hints(const mpcx_ctx *ctx, int32_t P) { return ctx->prev_cut + P; }

// log: the run log's descriptor or nullptr = none (then exactly the launches of a step without one)
// o: the options (never nullptr here).  MPCX_STOP_SPEED changes three arguments of a step and no launch: the conflict search reads the length
// of the previous tmp_trajectory from o->prev_len (0 before the batch's first step, the path length afterwards -- the window kernel sets it,
// device memory, so a replayed graph sees it change), its cut index in c->cut_len is the window stage's stop index over the whole path, and
// the record stage tests the goal against the whole path.
// r: retirement at the goal or nullptr = none (then exactly the launches of a step without it, with the same arguments).  With it every
// stage gets r->done: the conflict search returns at once for a retired agent and does not file it, the window stage gives it no place in
// the order and leaves the length of the queue in a spare word of ctx->ticket (the plant kernel zeroes it with the others), both solvers
// draw tickets up to that length, the rollout, the plant and the record stage skip the agent, and retire_kernel ends the step.  The pool
// row of a retired agent is still packed (by predict_kernel, or by pack_pool_kernel in the agent-sharded layout) from its frozen state and
// zero controls, and the scripted cars step as ever.
// sc: the scene (departure) or nullptr = none (then exactly the launches of a step with retirement alone, with the same arguments).  With it
// the prediction skips absent pool rows, the conflict search runs its SCENE instantiation on the list of present rows, the record stage's
// clearance leaves absent rows out, and retire_kernel sets absent[obs_skip[q]] for an agent that arrives -- the last launch of the step,
// so the others see the car gone from the next step on.
// ad: admission or nullptr = none (then exactly the launches of a step with a scene, with the same arguments).  With it the step BEGINS with the
// two launches of mpcx_admit.hip: a waiting agent (done[q] = 1, its own row absent) that is due and whose start pose is clear has both words
// cleared before the rollout is forked -- the side stream's rollout already reads done --, so every stage of this step drives and sees it.
// rs: respawn or nullptr = none (then exactly the launches of a step with admission, with the same arguments).  With it the step ENDS with
// respawn_kernel, after retire_kernel: an agent that has arrived leaves an episode record and, while its slot has vehicles left, is reset to
// the first step of a fresh batch and waits for the gate (wait >= 0).  The next step's rollout is forked after this launch in stream order.
// rt: routes or nullptr = none (then exactly the launches of a step with respawn, with the same arguments).  With them respawn_route_kernel
// takes respawn_kernel's place -- the same number of launches --: the reset also writes the next vehicle's route into c->path_off / c->path_len
// and its own start pose and index, which every stage of the next step reads afresh.
// pc: right of way or nullptr = none (then exactly the launches of a step with routes, with the same arguments).  With it the prediction also
// stores the standing records and the conflict search runs its PREC instantiation; in MPCX_PRECEDENCE_ENTRY one more launch,
// precedence_stamp_kernel, follows the admission stage -- before the prediction, so an agent admitted in this step is seen with its word.
// sg: traffic signals or nullptr = none (then exactly the launches of a step with right of way, with the same arguments).  With them one more
// launch, signal_kernel, follows the conflict search: it advances every agent's clock and, for an agent its light holds, lowers c->cut_len
// (the cut length, the stop index in speed mode) to the agent's stop line before the window stage reads it.  The agent is filed in the QP
// work queue already, under a key from the cut before this launch: the order of the queue only.
// av: vehicle-actuated signals or nullptr = none (then exactly the launches of a step with signals, with the same arguments).  With them
// actuated_signal_kernel stands in the place of signal_kernel -- the same number of launches --: a controller per junction decides the
// lights from the agents in front of their lines, the hold is signal_kernel's.
static int32_t enqueue_step(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const mpcx_run_log *log,
                            const mpcx_closed_loop_opts *o, const mpcx_retire *r, const mpcx_scene *sc, const mpcx_admit *ad,
                            const mpcx_respawn *rs, const mpcx_routes *rt, const mpcx_precedence *pc, const mpcx_signals *sg,
                            const mpcx_actuation *av) {
    const int P = c->P;
    const int32_t *done = r ? r->done : nullptr;
    int32_t *queue_len = r ? ctx->ticket + MPCX_TICKET_QUEUE_LEN : nullptr;
    const bool speed = o->stop_mode == MPCX_STOP_SPEED;
    ctx->bins_clean = false;        // until the plant kernel of this step is enqueued
    int32_t rc, pool_rows = P;
    if (ad) {       // (validated: a scene, retirement, the local pool)
        const int32_t na = c->n_actors > 0 ? c->n_actors : 0;
        rc = mpcx_admit_enqueue(ctx, ip, P, c->state, c->obs_off, c->obs_cnt, c->obs_skip, r->done, sc->n_rows, sc->absent, na, c->actors,
                                c->actor_state, c->tape, c->tape_rows, c->actor_row, ad);
        if (rc != MPCX_OK) return rc;
        if (pc && pc->mode == MPCX_PRECEDENCE_ENTRY) {      // (validated: ENTRY has admission)
            rc = mpcx_precedence_enqueue(ctx, P, c->obs_off, c->obs_skip, ad, pc);
            if (rc != MPCX_OK) return rc;
        }
    }
    // the warm-start rollout of this step needs only the states and the previous solution: it runs on the side stream BESIDE the pool pack,
    // the prediction and the conflict search (a chain of T dependent sincos / tan per agent, 35-45 us) and is joined by the window selection
    rc = mpcx_rollout_fork(ctx, P, c->state, c->u_sol, c->xbar, done);
    if (rc != MPCX_OK) return rc;
    // the conflict search leaves the cut lengths of the previous step in ctx->prev_cut (the queue of the QP kernel puts the agents whose
    // cut moved at the front) and files every agent under its work-queue key (previous iteration count + "the cut moved"): hard problems first.  The window
    // selection then writes the queue order and the plant kernel resets bins and ticket, so the counting sort costs no launch of its own.
    const bool binned = P < (1 << 24);
    mpcx_interaction_extras ix;
    ix.prev_save = ctx->prev_cut;
    ix.near = near_hints(ctx, P);
    ix.bin_hint = binned ? c->iters : nullptr;
    ix.done = done;
    ix.absent = sc ? sc->absent : nullptr;
    if (pc) { ix.prec = pc->prec; ix.stand = pc->stand; }       // (validated: a scene)
    if (speed) ix.key_prev = c->cut_len;        // "the cut moved" = the stop index moved
    if (c->exchange == MPCX_SHARD_AGENTS) {
        // agent-sharded layout: this rank's rows travel to every rank, every rank assembles the whole pool (one RCCL all-gather)
        mpcx::PackArgs pa{P, c->state, c->applied, c->obs_local};
        hipLaunchKernelGGL(mpcx::pack_pool_kernel, dim3((P + 63) / 64), dim3(64), 0, ctx->stream, pa);
        rc = mpcx_allgather_states(ctx, MPCX_SHARD_AGENTS, c->n_inst, c->agents_local, c->obs_local, c->obs6);
        if (rc != MPCX_OK) return rc;
        pool_rows = P * ctx->comm_world;
    } else {
        // local pool: row q is agent q, and the prediction kernel (inside the conflict search's stage) packs it on its way -- no launch of its own
        ix.pack_state = c->state; ix.pack_applied = c->applied;
        if (c->n_actors > 0) {
            // scripted traffic (mpc_intersection.py:118-122): the actors' get() rows go into their pool rows and their step() is taken at once --
            // it shows in the NEXT step's rows, as o.step() at the end of the reference's loop body does (:155-156).  Agent q sits in row ego_row[q].
            rc = mpcx_traffic_enqueue(ctx, c->n_actors, c->actors, c->actor_state, c->tape, c->tape_rows, c->actor_row, c->pool_rows, c->obs6);
            if (rc != MPCX_OK) return rc;
            ix.ego_row = c->ego_row; ix.actor_row = c->actor_row;
            ix.n_ego = P; ix.n_actors = c->n_actors;
            pool_rows = c->pool_rows;
        }
    }
    rc = mpcx_interaction_enqueue(ctx, ip, P, c->state, c->path_xyyaw, c->path_cs, c->path_off, c->path_len,
                                  speed ? o->prev_len : c->cut_len /* previous step's cut; read before it is rewritten */, pool_rows, c->obs6,
                                  c->obs_off, c->obs_cnt, c->obs_skip, c->traj_idx, c->hit_idx, c->hit_xy, c->cut_len, ix);
    if (rc != MPCX_OK) return rc;
    if (sg) {       // (validated: the local pool, one linearisation pass)
        rc = av ? mpcx_actuated_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, sg, av)
                : mpcx_signal_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, sg);
        if (rc != MPCX_OK) return rc;
    }
    // lib/mpc.py:226-237: MAX_ITER passes of (reference window, rollout, QP); from the second pass on the window is spaced by the
    // previous pass's speeds (row 2 of its x) and the rollout uses its inputs.  (Where a pass fails the reference crashes in the next
    // one -- zip over None; here the next pass starts from the untouched warm start, as after a failed step.)
    const int Wd = ctx->mpc.T + 1;
    for (int pass = 0; pass < ctx->lin_passes; pass++) {
        const bool first = pass == 0;
        // the first pass writes the queue order and joins the rollout forked above; a later one forks its own
        mpcx_window_extras wx{binned && first, near_hints(ctx, P), c->traj_idx, first};
        if (speed) { wx.stop_idx = c->cut_len; wx.v_ref = o->v_ref; wx.len_seen = o->prev_len; }
        wx.done = done; wx.queue_len = queue_len;       // (retirement is refused with more than one pass or without bins)
        rc = mpcx_window_enqueue(ctx, P, c->state, c->u_sol, c->path_xyyaw, c->path_v, c->path_off, speed ? c->path_len : c->cut_len, c->dl,
                                 c->target_ind, pass ? c->x_sol + 2 * Wd : nullptr, 4 * (int64_t)Wd, c->xref, c->reaches_end, c->xbar, wx);
        if (rc != MPCX_OK) return rc;
        // (further linearisation passes build their order in line, from the iteration counts of the pass before)
        const mpcx_qp_order ord{binned && first, c->iters, c->cut_len, ctx->prev_cut, queue_len};
        rc = mpcx_qp_enqueue(ctx, P, c->state, c->xref, c->xbar, c->reaches_end, c->u_sol, c->x_sol, c->u_sol, c->status, c->iters, c->kkt, ord);
        if (rc != MPCX_OK) return rc;
    }
    const mpcx_plant_extras px{c->iters, binned, done};
    rc = mpcx_plant_enqueue(ctx, P, c->state, c->u_sol, c->status, c->applied, px);
    if (rc == MPCX_OK) ctx->bins_clean = binned;
    if (rc != MPCX_OK) return rc;
    // the run log: one row per agent from the buffers as the step leaves them; the pool still holds the rows this step's conflict search saw
    if (log) {
        rc = mpcx_record_enqueue(ctx, ip, P, c->state, c->applied, c->x_sol, c->path_xyyaw, c->path_off, c->path_len, c->target_ind, c->cut_len,
                                 c->traj_idx, c->hit_idx, c->status, c->iters, pool_rows, c->obs6, c->obs_off, c->obs_cnt, c->obs_skip, log,
                                 speed ? c->path_len : nullptr, done, sc ? sc->absent : nullptr);
        if (rc != MPCX_OK) return rc;
    }
    // retirement: the goal test of the record stage (len(cx) = cut_len, the whole path in speed mode), after it, so that the arrival
    // step's row logs the controls really applied
    if (r) rc = mpcx_retire_enqueue(ctx, P, c->state, c->applied, c->path_xyyaw, c->path_off, c->path_len, c->target_ind,
                                    speed ? c->path_len : c->cut_len, r, sc, c->obs_skip);
    if (rc != MPCX_OK) return rc;
    if (rs && rt)   // (validated: respawn, and the descriptor's own path_off / path_len)
        rc = mpcx_route_enqueue(ctx, P, c->state, c->applied, c->u_sol, c->traj_idx, c->target_ind, c->cut_len, c->iters,
                                speed ? o->prev_len : nullptr, c->obs_skip, sc->n_rows, log, r, ad, rs, rt);
    else if (rs)    // (validated: admission, and with it a scene and retirement)
        rc = mpcx_respawn_enqueue(ctx, P, c->state, c->applied, c->u_sol, c->traj_idx, c->target_ind, c->cut_len, c->iters,
                                  speed ? o->prev_len : nullptr, c->obs_skip, sc->n_rows, log, r, ad, rs);
    return rc;
}

// A run of n_steps with step fusion (mpcx_set_step_fusion; closed_loop_run decides where it applies: the local pool, no scripted traffic, one
// linearisation pass, no optional stage): per step ONE launch for what belongs to an agent alone -- the plant update of the step before
// (from the second step of the run on), the pack and prediction of its pool row, its warm-start rollout -- then the conflict search, the
// window selection and the solve with the arguments enqueue_step gives them; the last step's plant update ends the run in a launch of its
// own.  Nothing runs on the side stream and neither event is touched.  The buffers hold the bits enqueue_step leaves.
static int32_t enqueue_fused_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const mpcx_closed_loop_opts *o,
                                 int32_t n_steps) {
    const int P = c->P;
    const bool speed = o->stop_mode == MPCX_STOP_SPEED;
    const bool binned = P < (1 << 24);
    int32_t rc;
    for (int s = 0; s < n_steps; s++) {
        ctx->bins_clean = false;        // until the plant update of this step is enqueued
        rc = mpcx_head_enqueue(ctx, ip, P, c->state, c->applied, c->u_sol, c->status, c->iters, c->xbar, c->obs6, s > 0, binned);
        if (rc != MPCX_OK) return rc;
        mpcx_interaction_extras ix;
        ix.prev_save = ctx->prev_cut;
        ix.near = near_hints(ctx, P);
        ix.bin_hint = binned ? c->iters : nullptr;
        if (speed) ix.key_prev = c->cut_len;
        ix.pack_state = c->state; ix.pack_applied = c->applied;
        ix.predicted = true;
        rc = mpcx_interaction_enqueue(ctx, ip, P, c->state, c->path_xyyaw, c->path_cs, c->path_off, c->path_len,
                                      speed ? o->prev_len : c->cut_len, P, c->obs6, c->obs_off, c->obs_cnt, c->obs_skip, c->traj_idx, c->hit_idx,
                                      c->hit_xy, c->cut_len, ix);
        if (rc != MPCX_OK) return rc;
        mpcx_window_extras wx{binned, near_hints(ctx, P), c->traj_idx, true};
        wx.rollout_done = true;
        if (speed) { wx.stop_idx = c->cut_len; wx.v_ref = o->v_ref; wx.len_seen = o->prev_len; }
        rc = mpcx_window_enqueue(ctx, P, c->state, c->u_sol, c->path_xyyaw, c->path_v, c->path_off, speed ? c->path_len : c->cut_len, c->dl,
                                 c->target_ind, nullptr, 4 * (int64_t)(ctx->mpc.T + 1), c->xref, c->reaches_end, c->xbar, wx);
        if (rc != MPCX_OK) return rc;
        const mpcx_qp_order ord{binned, c->iters, c->cut_len, ctx->prev_cut, nullptr};
        rc = mpcx_qp_enqueue(ctx, P, c->state, c->xref, c->xbar, c->reaches_end, c->u_sol, c->x_sol, c->u_sol, c->status, c->iters, c->kkt, ord);
        if (rc != MPCX_OK) return rc;
    }
    const mpcx_plant_extras px{c->iters, binned, nullptr};
    rc = mpcx_plant_enqueue(ctx, P, c->state, c->u_sol, c->status, c->applied, px);
    if (rc == MPCX_OK) ctx->bins_clean = binned;
    return rc;
}

static int32_t closed_loop_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const mpcx_run_log *log,
                               const mpcx_closed_loop_opts *opts, const mpcx_retire *retire, const mpcx_scene *scene, const mpcx_admit *admit,
                               const mpcx_respawn *respawn, const mpcx_routes *routes, const mpcx_precedence *precedence,
                               const mpcx_signals *signals, const mpcx_actuation *actuation, int32_t n_steps, int32_t use_graph) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (!ip || !c || n_steps < 0 || c->P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: null descriptor or negative count");
    // the options as the graph's key holds them: nullptr and a cut-mode struct, whatever its other fields say, are the same run
    mpcx_closed_loop_opts opt = {};
    if (opts && opts->stop_mode != MPCX_STOP_CUT) {     // refused before anything is launched, whatever n_steps is
        if (opts->stop_mode != MPCX_STOP_SPEED)
            return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: unknown stop mode %d (MPCX_STOP_CUT or MPCX_STOP_SPEED)", opts->stop_mode);
        if (!std::isfinite(opts->v_ref)) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: MPCX_STOP_SPEED with a speed reference v_ref that is not finite");
        if (!opts->prev_len) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: MPCX_STOP_SPEED needs prev_len (P zero-initialised int32)");
        opt.stop_mode = MPCX_STOP_SPEED; opt.v_ref = opts->v_ref; opt.prev_len = opts->prev_len;
    }
    if (mpcx_record_absent(log)) log = nullptr;
    if (log) {          // refused before anything is launched, whatever n_steps is
        const int32_t lrc = mpcx_record_validate(ctx, log, c->obs_skip);
        if (lrc != MPCX_OK) return lrc;
    }
    if (mpcx_retire_absent(retire)) retire = nullptr;
    if (retire) {       // refused before anything is launched, whatever n_steps is
        const int32_t rrc = mpcx_retire_validate(ctx, retire, c->P);
        if (rrc != MPCX_OK) return rrc;
    }
    if (mpcx_scene_absent(scene)) scene = nullptr;
    if (scene) {        // refused before anything is launched, whatever n_steps is
        const bool traffic = c->n_actors > 0;
        const size_t rows = traffic ? (size_t)(c->pool_rows > 0 ? c->pool_rows : 0) : (size_t)c->P;
        int32_t src = mpcx_scene_validate(ctx, scene, retire, c->exchange, rows, c->obs_skip);
        if (src == MPCX_OK && c->P > 0) src = mpcx_loop_check_rows(ctx, c->P, c->obs_skip, scene->n_rows, "scene");
        if (src != MPCX_OK) return src;
    }
    if (mpcx_admit_absent(admit)) admit = nullptr;
    if (admit) {        // refused before anything is launched, whatever n_steps is
        const int32_t arc = mpcx_admit_validate(ctx, admit, retire, scene, c->exchange);
        if (arc != MPCX_OK) return arc;
    }
    if (mpcx_respawn_absent(respawn)) respawn = nullptr;
    if (respawn) {      // refused before anything is launched, whatever n_steps is
        const int32_t prc = mpcx_respawn_validate(ctx, respawn, admit);
        if (prc != MPCX_OK) return prc;
    }
    if (mpcx_routes_absent(routes)) routes = nullptr;
    if (routes) {       // refused before anything is launched, whatever n_steps is
        // the longest route the conflict search handles: max_path_len as mpcx_interaction_enqueue rounds it
        int32_t cap = ip->max_path_len > 0 ? ip->max_path_len : MPCX_MAX_REMAINING;
        if (cap < 512) cap = 512;
        cap = (cap + 63) / 64 * 64;
        const int32_t trc = mpcx_routes_validate(ctx, routes, respawn, c->path_off, c->path_len, cap);
        if (trc != MPCX_OK) return trc;
    }
    if (mpcx_precedence_absent(precedence)) precedence = nullptr;
    if (precedence) {   // refused before anything is launched, whatever n_steps is
        const int32_t prc = mpcx_precedence_validate(ctx, precedence, scene, admit);
        if (prc != MPCX_OK) return prc;
    }
    if (mpcx_signals_absent(signals)) signals = nullptr;
    if (mpcx_actuation_absent(actuation)) actuation = nullptr;
    mpcx_actuation act;         // by value with its padding zeroed: the cached graph's key
    memset(&act, 0, sizeof act);
    if (actuation) {    // refused before anything is launched, whatever n_steps is; checks the signals it draws on too
        const int32_t arc = mpcx_actuation_validate(ctx, actuation, signals, c->P, c->exchange);
        if (arc != MPCX_OK) return arc;
        act.phase_groups = actuation->phase_groups; act.phase_time = actuation->phase_time; act.ctrl_time = actuation->ctrl_time;
        act.ctrl_of = actuation->ctrl_of; act.jstate = actuation->jstate; act.lights = actuation->lights; act.calls = actuation->calls;
        act.n_per = actuation->n_per; act.n_junctions = actuation->n_junctions; act.n_phases = actuation->n_phases;
        act.n_ctrl = actuation->n_ctrl;
        actuation = &act;
    } else if (signals) {      // refused before anything is launched, whatever n_steps is
        const int32_t grc = mpcx_signals_validate(ctx, signals, c->exchange);
        if (grc != MPCX_OK) return grc;
    }
    if (n_steps == 0 || c->P == 0) return MPCX_OK;
    if (!c->state || !c->applied || !c->obs6 || !c->path_xyyaw || !c->path_cs || !c->path_off || !c->path_len ||
        !c->obs_off || !c->obs_cnt || !c->traj_idx || !c->target_ind || !c->hit_idx || !c->cut_len || !c->hit_xy ||
        !c->xref || !c->xbar || !c->reaches_end || !c->x_sol || !c->u_sol || !c->status || !c->iters || !c->kkt || !(c->dl > 0))
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: null buffer in the descriptor or dl <= 0");
    if (ip->pred_steps < 1 || ip->pred_steps > MPCX_PRED_STEPS_MAX)
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: pred_steps outside 1..%d", MPCX_PRED_STEPS_MAX);
    if (c->exchange != 0 && c->exchange != MPCX_SHARD_AGENTS)
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: exchange must be 0 or MPCX_SHARD_AGENTS");
    if (c->exchange == MPCX_SHARD_AGENTS) {
        if (!c->obs_local || c->n_inst < 0 || c->agents_local < 0 || (long)c->n_inst * c->agents_local != (long)c->P)
            return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: agent-sharded layout needs obs_local and P = n_inst * agents_local");
        if (use_graph) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: the agent-sharded layout (RCCL exchange) is not captured into a graph");
    }
    if (c->n_actors < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: negative number of scripted actors");
    if (c->n_actors > 0) {
        if (c->exchange == MPCX_SHARD_AGENTS)
            return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: scripted traffic is not supported in the agent-sharded layout (it is instance-local: shard by instances)");
        if (!c->actors || !c->actor_state || !c->actor_row || !c->ego_row || c->tape_rows < 0 || (long)c->pool_rows < (long)c->P + c->n_actors)
            return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: scripted traffic needs actors, actor_state, actor_row, ego_row and pool_rows >= P + n_actors");
    }
    // everything that allocates (or reads back) happens before the first launch (and outside any capture)
    const size_t pool_rows = c->n_actors > 0 ? (size_t)c->pool_rows : (size_t)c->P * (c->exchange == MPCX_SHARD_AGENTS ? (size_t)ctx->comm_world : 1);
    int32_t rc = mpcx_ensure_pred(ctx, pool_rows * ip->pred_steps * 4);
    if (rc != MPCX_OK) return rc;
    if (c->n_actors > 0) {
        rc = mpcx_traffic_validate(ctx, c->n_actors, c->actors, c->tape, c->tape_rows, c->actor_row, c->pool_rows);
        if (rc != MPCX_OK) return rc;
        rc = mpcx_loop_check_rows(ctx, c->P, c->ego_row, c->pool_rows);
        if (rc != MPCX_OK) return rc;
    }
    rc = mpcx_ensure_ticket(ctx);
    if (rc != MPCX_OK) return rc;
    if (admit) {
        rc = mpcx_admit_prepare(ctx, (size_t)scene->n_rows);
        if (rc != MPCX_OK) return rc;
    }
    {
        const size_t slots = ((size_t)c->P + 63) / 64;
        if (slots > ctx->stats_slots) {         // a larger batch: the counters so far are folded into slot 0 of the new table
            int64_t keep[4] = {0, 0, 0, 0};
            if (ctx->stats) { rc = mpcx_closed_loop_stats(ctx, keep, 0); if (rc != MPCX_OK) return rc; (void)hipFree(ctx->stats); ctx->stats = nullptr; ctx->stats_slots = 0; }
            if (hipMalloc((void **)&ctx->stats, 4 * slots * sizeof(unsigned long long)) != hipSuccess ||
                hipMemsetAsync(ctx->stats, 0, 4 * slots * sizeof(unsigned long long), ctx->stream) != hipSuccess ||
                hipMemcpyAsync(ctx->stats, keep, sizeof keep, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess)
                return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: cannot allocate the run statistics");
            ctx->stats_slots = slots;
        }
    }
    rc = mpcx_ensure_order(ctx, (size_t)c->P);
    if (rc != MPCX_OK) return rc;
    {       // queue bins: counters + (key, slot) per agent.  The plant kernel leaves counters and ticket zeroed step by step; they are
            // filled here only when the host cannot know that (first run, a step that failed half way, a solve outside the loop since)
        const size_t need = (size_t)MPCX_ORDER_COPIES * MPCX_ORDER_BINS + (size_t)c->P;
        if (need * sizeof(int32_t) > ctx->bins_cap) ctx->bins_clean = false;
        rc = mpcx_grow(ctx, (void **)&ctx->bins, &ctx->bins_cap, need * sizeof(int32_t), "the queue bins");
        if (rc != MPCX_OK) return rc;
        if (!ctx->bins_clean) {
            if (hipMemsetAsync(ctx->bins, 0, (size_t)MPCX_ORDER_COPIES * MPCX_ORDER_BINS * sizeof(int32_t), ctx->stream) != hipSuccess ||
                hipMemsetAsync(ctx->ticket, 0, MPCX_TICKET_WORDS * sizeof(int32_t), ctx->stream) != hipSuccess)
                return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipMemsetAsync failed");
            ctx->bins_clean = true;
        }
    }
    rc = mpcx_grow(ctx, (void **)&ctx->prev_cut, &ctx->prev_cut_cap, 4 * (size_t)c->P * sizeof(int32_t), "the previous cut lengths");   // P cut lengths | near_hints
    if (rc != MPCX_OK) return rc;

    if (!use_graph) {
        if (ctx->step_fusion && c->exchange == 0 && c->n_actors == 0 && ctx->lin_passes == 1 && !log && !retire && !scene && !admit && !respawn &&
            !routes && !precedence && !signals && !actuation)
            return enqueue_fused_run(ctx, ip, c, &opt, n_steps);
        for (int s = 0; s < n_steps; s++) {
            rc = enqueue_step(ctx, ip, c, log, &opt, retire, scene, admit, respawn, routes, precedence, signals, actuation);
            if (rc != MPCX_OK) return rc;
        }
        return MPCX_OK;
    }

    if (!ctx->stream) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: graph replay needs a non-default stream");
    if (ctx->prof_qp)       // the event pairs of mpcx_profile_qp cannot be recorded inside a replayed graph: say so instead of reporting 0 launches
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: mpcx_profile_qp is on; the QP launches of a replayed graph are not bracketed by events -- run without graph or switch the hook off");
    unsigned char key[sizeof ctx->loop_key];
    static_assert(sizeof(mpcx_closed_loop) + sizeof(mpcx_run_log) + sizeof(mpcx_closed_loop_opts) + sizeof(mpcx_retire) + sizeof(mpcx_scene) + sizeof(mpcx_admit) + sizeof(mpcx_respawn) + sizeof(mpcx_routes) + sizeof(mpcx_precedence) + sizeof(mpcx_signals) + sizeof(mpcx_actuation) + sizeof(mpcx_interaction_params) +
                  sizeof(mpcx_mpc_params) + 10 * sizeof(void *) <= sizeof key,
                  "loop_key too small");
    memset(key, 0, sizeof key);
    size_t o = 0;
    memcpy(key + o, c, sizeof *c); o += sizeof *c;
    if (log) memcpy(key + o, log, sizeof *log);     // (zeros = no log: a graph captured without the record stage)
    o += sizeof *log;
    memcpy(key + o, &opt, sizeof opt); o += sizeof opt;
    if (retire) memcpy(key + o, retire, sizeof *retire);     // (zeros = no retirement: a graph captured without it)
    o += sizeof *retire;
    if (scene) memcpy(key + o, scene, sizeof *scene);        // (zeros = no scene: a graph captured without departure)
    o += sizeof *scene;
    if (admit) memcpy(key + o, admit, sizeof *admit);        // (zeros = no admission: a graph captured without its two launches)
    o += sizeof *admit;
    if (respawn) memcpy(key + o, respawn, sizeof *respawn);  // (zeros = no respawn: a graph captured without its launch)
    o += sizeof *respawn;
    if (routes) memcpy(key + o, routes, sizeof *routes);     // (zeros = no routes: a graph captured with respawn_kernel)
    o += sizeof *routes;
    if (precedence) memcpy(key + o, precedence, sizeof *precedence);     // (zeros = no precedence: a graph captured without its instantiations)
    o += sizeof *precedence;
    if (signals) memcpy(key + o, signals, sizeof *signals);  // (zeros = no signals: a graph captured without signal_kernel)
    o += sizeof *signals;
    if (actuation) memcpy(key + o, actuation, sizeof *actuation);    // (zeros = no actuation: a graph captured with signal_kernel, if any)
    o += sizeof *actuation;
    memcpy(key + o, &ctx->admit_tab, sizeof ctx->admit_tab); o += sizeof ctx->admit_tab;
    memcpy(key + o, ip, sizeof *ip); o += sizeof *ip;
    memcpy(key + o, &ctx->mpc, sizeof ctx->mpc); o += sizeof ctx->mpc;
    memcpy(key + o, &ctx->pred, sizeof ctx->pred); o += sizeof ctx->pred;
    memcpy(key + o, &ctx->tune, sizeof ctx->tune); o += sizeof ctx->tune;
    memcpy(key + o, &ctx->order, sizeof ctx->order); o += sizeof ctx->order;
    memcpy(key + o, &ctx->prev_cut, sizeof ctx->prev_cut); o += sizeof ctx->prev_cut;
    memcpy(key + o, &ctx->bins, sizeof ctx->bins); o += sizeof ctx->bins;
    memcpy(key + o, &ctx->qp_solver, sizeof ctx->qp_solver); o += sizeof ctx->qp_solver;      // the captured launch is the solver chosen at capture time
    memcpy(key + o, &ctx->lin_passes, sizeof ctx->lin_passes); o += sizeof ctx->lin_passes;
    memcpy(key + o, &ctx->stats, sizeof ctx->stats);
    if (!ctx->loop_exec || memcmp(key, ctx->loop_key, sizeof key) != 0) {
        if (ctx->loop_exec) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipGraphExecDestroy(ctx->loop_exec);
            ctx->loop_exec = nullptr;
        }
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipStreamBeginCapture failed");
        rc = enqueue_step(ctx, ip, c, log, &opt, retire, scene, admit, respawn, routes, precedence, signals, actuation);
        hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
        if (rc != MPCX_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess || !graph) return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: stream capture failed: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&ctx->loop_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { ctx->loop_exec = nullptr; return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipGraphInstantiate: %s", hipGetErrorString(e)); }
        memcpy(ctx->loop_key, key, sizeof key);
    }
    for (int s = 0; s < n_steps; s++)
        if (hipGraphLaunch(ctx->loop_exec, ctx->stream) != hipSuccess)
            return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipGraphLaunch failed");
    return MPCX_OK;
}

extern "C" int32_t mpcx_closed_loop_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                        int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_logged(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, log, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_opts(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                             const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, log, opts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_retire(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                               int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, log, opts, retire, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_scene(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                              const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                              const mpcx_scene *scene, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, log, opts, retire, scene, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_admit(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                              const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                              const mpcx_scene *scene, const mpcx_admit *admit, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, log, opts, retire, scene, admit, nullptr, nullptr, nullptr, nullptr, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_respawn(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                int32_t n_steps, int32_t use_graph) {
    return mpcx_closed_loop_run_routes(ctx, ip, c, log, opts, retire, scene, admit, respawn, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_routes(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                               const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                               const mpcx_routes *routes, int32_t n_steps, int32_t use_graph) {
    return mpcx_closed_loop_run_precedence(ctx, ip, c, log, opts, retire, scene, admit, respawn, routes, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_precedence(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                   const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                   const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                   const mpcx_routes *routes, const mpcx_precedence *precedence, int32_t n_steps,
                                                   int32_t use_graph) {
    return mpcx_closed_loop_run_signals(ctx, ip, c, log, opts, retire, scene, admit, respawn, routes, precedence, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_signals(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                                int32_t n_steps, int32_t use_graph) {
    return mpcx_closed_loop_run_actuated(ctx, ip, c, log, opts, retire, scene, admit, respawn, routes, precedence, signals, nullptr, n_steps, use_graph);
}

extern "C" int32_t mpcx_closed_loop_run_actuated(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                 const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                 const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                 const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                                 const mpcx_actuation *actuation, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, log, opts, retire, scene, admit, respawn, routes, precedence, signals, actuation, n_steps, use_graph);
}
