// mpcx_loop.hip -- the reference's scenario loop body (main/scenarios/mpc_intersection.py:95-159) for P agents as a
// device-resident pipeline (and, with MPCX_STOP_SPEED, that of main/scenarios/mpc_intersection_new_ref.py:90-159: the same stages, the
// path kept whole and the speed reference zeroed from the conflict on):
// n_steps x [scripted traffic rows -> pool pack -> predict -> conflict search + path cut -> reference window ->
// rollout -> QP -> plant (-> run-log record, iff a log is attached)], enqueued back to back on the context's stream (optionally as a replayed hipGraph), no
// host synchronisation or host arithmetic in between.  mpcx::LoopStages lists the optional stages: the launches each adds, what it needs.
// Every stage is the kernel behind the per-stage C entry point, called with the very buffers the descriptor names, so a run is bit-identical
// to driving the stages one by one from the host.  With step fusion (mpcx_set_step_fusion, enqueue_fused_run) a run without any of the optional stages takes the plant
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

// What the caller of an entry point passed beside the descriptor, in the order the entry points grew; nullptr = nothing.
struct LoopArgs {
    const mpcx_run_log *log; const mpcx_closed_loop_opts *opts; const mpcx_retire *retire; const mpcx_scene *scene; const mpcx_admit *admit;
    const mpcx_respawn *respawn; const mpcx_routes *routes; const mpcx_precedence *precedence; const mpcx_signals *signals;
    const mpcx_actuation *actuation; const mpcx_advice *advice; const mpcx_intent *intent; const mpcx_reservation *reservation;
};

// The optional stages of a run, checked (check_stages): a pointer is nullptr where the stage is off -- NULL and what the stage's own
// mpcx_*_absent calls "none" are the same run --, and a step without a stage is exactly the launches of a step that never heard of it, with
// the same arguments.
struct LoopStages {
    // the run log: mpcx_record_enqueue behind the plant update, one row per agent from the buffers as the step leaves them (the pool still
    // holds the rows this step's conflict search saw)
    const mpcx_run_log *log = nullptr;
    // by value: nullptr and a cut-mode struct, whatever its other fields say, are the same run.  MPCX_STOP_SPEED changes three arguments of
    // a step and no launch: the conflict search reads the length of the previous tmp_trajectory from prev_len (0 before the batch's first
    // step, the path length afterwards -- the window kernel sets it, device memory, so a replayed graph sees it change), its cut index in
    // c->cut_len is the window stage's stop index over the whole path, and the record stage tests the goal against the whole path.
    mpcx_closed_loop_opts opts = {};
    // retirement at the goal: retire_kernel behind the record stage (so the arrival step's row logs the controls really applied).  Every
    // stage gets retire->done: the conflict search returns at once for a retired agent and does not file it, the window stage gives it no
    // place in the order and leaves the length of the queue in a spare word of ctx->ticket (the plant kernel zeroes it with the others),
    // both solvers draw tickets up to that length, the rollout, the plant and the record stage skip the agent.  Its pool row is still packed
    // from its frozen state and zero controls, and the scripted cars step as ever.  Refused with more than one linearisation pass.
    const mpcx_retire *retire = nullptr;
    // departure, no launch of its own; needs retirement and the local pool.  The prediction skips absent pool rows, the conflict search runs
    // its SCENE instantiation on the list of present rows, the record stage's clearance leaves absent rows out, and retire_kernel sets
    // absent[obs_skip[q]] for an agent that arrives -- the last launch of the step, so the others see the car gone from the next step on.
    const mpcx_scene *scene = nullptr;
    // admission: the step BEGINS with the two launches of mpcx_admit.hip; needs a scene.  A waiting agent (done[q] = 1, its own row absent)
    // that is due and whose start pose is clear has both words cleared before the rollout is forked -- the side stream's rollout already
    // reads done --, so every stage of this step drives and sees it.
    const mpcx_admit *admit = nullptr;
    // respawn: the step ENDS with respawn_kernel, behind retire_kernel; needs admission.  An agent that has arrived leaves an episode record
    // and, while its slot has vehicles left, is reset to the first step of a fresh batch and waits for the gate (wait >= 0).  The next
    // step's rollout is forked after this launch in stream order.
    const mpcx_respawn *respawn = nullptr;
    // routes: respawn_route_kernel in respawn_kernel's place; needs respawn and the descriptor's own path_off / path_len.  The reset also
    // writes the next vehicle's route into them and its own start pose and index, which every stage of the next step reads afresh.
    const mpcx_routes *routes = nullptr;
    // right of way, needs a scene: the prediction also stores the standing records and the conflict search runs its PREC instantiation.  In
    // MPCX_PRECEDENCE_ENTRY, which needs admission, precedence_stamp_kernel follows the admission stage -- before the prediction, so an
    // agent admitted in this step is seen with its word.
    const mpcx_precedence *precedence = nullptr;
    // traffic signals: signal_kernel between the conflict search and the window stage; needs the local pool and one linearisation pass.  It
    // advances every agent's clock and, for an agent its light holds, lowers c->cut_len (the cut length, the stop index in speed mode) to
    // the agent's stop line before the window stage reads it.  The agent is filed in the QP work queue already, under a key from the cut
    // before this launch: the order of the queue only.
    const mpcx_signals *signals = nullptr;
    // vehicle-actuated signals: actuated_signal_kernel in signal_kernel's place; needs signals.  A controller per junction decides the
    // lights from the agents in front of their lines, the hold is signal_kernel's.  By value with its padding zeroed (all zeros where
    // `actuated` is false): the cached graph's key takes it as it stands.
    mpcx_actuation actuation;
    bool actuated = false;
    // signal-aware approach speed: advise_kernel between the window stage and the QP; needs signals under a fixed plan (no actuation) and
    // MPCX_STOP_SPEED.  It caps row 2 of c->xref for an agent that would reach its stop line on red and writes advice->advised; the QP
    // reads the capped window.  Signals allow one linearisation pass, so there is one window stage to follow.
    const mpcx_advice *advice = nullptr;
    // shared plans: intent_kernel between the prediction and the conflict search (inside mpcx_interaction_enqueue); needs the local pool and
    // obs_skip.  It overwrites the predicted frames of a sharing agent's own pool row with its plan of the step before (c->u_sol, which no
    // stage has touched yet) re-rolled through the prediction's model, and writes intent->frames.  Never with step fusion: none() is false.
    const mpcx_intent *intent = nullptr;
    // crossing reservations: reserve_kernel in signal_kernel's place; needs signals without a plan, and neither actuation nor advice.  A
    // manager per junction admits an agent only if its movement conflicts with none that holds the crossing; the hold is signal_kernel's.
    const mpcx_reservation *reserve = nullptr;
    // car following (mpcx_set_following: it attaches to the context, not to an entry point): follow_kernel behind the signal / actuated /
    // reserve stage, or behind the conflict search where there are no signals; needs the local pool.  It lowers c->cut_len to a stop point
    // behind the agent's leader before the window stage reads it and writes leader, gap and cap; in MPCX_STOP_SPEED follow_clamp_kernel
    // behind every window stage (and the advice stage) caps row 2 of c->xref.  &ctx->following while on.
    const mpcx_following *follow = nullptr;
    // the near-miss log (mpcx_set_safety: it attaches to the context too): safety_kernel directly behind the conflict search, before the
    // hold; needs the local pool and obs_skip.  It reads obs6, ctx->pred and traj_idx as the conflict search left them and writes only the
    // struct's own words: no other launch of the step sees it.  &ctx->safety while on.
    const mpcx_safety *safety = nullptr;
    // line of sight (mpcx_set_sight: it attaches to the context too): sight_kernel inside the conflict search's stage, behind the pack of
    // the pool and the intent stage, and the SIGHT instantiation of the conflict search; needs retirement, a scene and obs_skip.
    // &ctx->sight while on.
    const mpcx_sight *sight = nullptr;
    // keep clear (mpcx_set_keepclear: it attaches to the context too): keepclear_kernel directly behind signal_kernel /
    // actuated_signal_kernel and in front of the following stage; needs signals and no reservation.  It reads held as the hold left it and,
    // for an agent whose light lets it go while a conflicting movement is inside the crossing, lowers c->cut_len to the agent's stop line.
    // &ctx->keepclear while on.
    const mpcx_keepclear *keepclear = nullptr;
    // priority road (mpcx_set_priority: it attaches to the context too): priority_kernel in the hold's place -- behind the conflict search
    // and the safety stage, in front of the following stage; refused beside signals, actuation or a reservation.  For an agent of a minor
    // movement that meets a conflicting car of smaller rank within its critical gap it lowers c->cut_len to the agent's stop line.
    // &ctx->priority while on.
    const mpcx_priority *priority = nullptr;
    // stop signs (mpcx_set_stopsign: it attaches to the context too): stopsign_kernel in the priority stage's place; refused beside signals,
    // actuation, a reservation or the priority road.  It holds an agent of a signed movement at its stop line until it has stood there and
    // its turn has come, by lowering c->cut_len to the line.  &ctx->stopsign while on.
    const mpcx_stopsign *stopsign = nullptr;
    // firm hold (mpcx_set_braking: it attaches to the context too): brake_mark_kernel behind the last hold stage and the following stage, in
    // front of the window stage; in MPCX_STOP_SPEED brake_clamp_kernel behind every window stage, beside the advice and following clamps.
    // Needs a source of stop lines (signals, actuation, a reservation, the priority road or stop signs), the local pool and one linearisation pass.  The
    // mark writes ctx->win_len, which the window stage is handed in place of path_len: a line-held agent's window ends on its stop point,
    // everybody else's length is path_len's.  `lines`: the table and the hold words of THIS run's stages.  &ctx->braking while on.
    const mpcx_braking *brake = nullptr;
    struct { const int32_t *path_stop, *held, *boxed, *yielding; int32_t n_points; } lines = {nullptr, nullptr, nullptr, nullptr, 0};

    LoopStages() { memset(&actuation, 0, sizeof actuation); }
    // no optional stage at all (the stop mode is none: it adds no launch): what step fusion asks for
    bool none() const { return !log && !retire && !scene && !admit && !respawn && !routes && !precedence && !signals && !actuated && !advice && !intent && !reserve && !follow && !safety && !sight && !keepclear && !priority && !stopsign && !brake; }
    bool speed() const { return opts.stop_mode == MPCX_STOP_SPEED; }
    const int32_t *done() const { return retire ? retire->done : nullptr; }
};

// Everything the cached one-step graph was captured for (ctx->loop_key): a run whose key differs in any byte captures afresh.  Filled after
// a memset, so padding and the struct of a stage that is off are zeros.
struct LoopKey {
    mpcx_closed_loop desc;
    mpcx_run_log log; mpcx_closed_loop_opts opts; mpcx_retire retire; mpcx_scene scene; mpcx_admit admit; mpcx_respawn respawn;
    mpcx_routes routes; mpcx_precedence precedence; mpcx_signals signals; mpcx_actuation actuation; mpcx_advice advice; mpcx_intent intent; mpcx_reservation reservation;
    mpcx_following following;
    mpcx_safety safety;
    mpcx_sight sight;
    mpcx_keepclear keepclear;
    mpcx_priority priority;
    mpcx_stopsign stopsign;
    mpcx_braking braking;
    mpcx_interaction_params ip;
    mpcx_mpc_params mpc;
    const void *admit_tab, *pred, *tune, *order, *prev_cut, *bins, *stats, *win_len;      // the context's scratch the launches were given
    int qp_solver, lin_passes, qp_plain_rounds;          // the captured launch is the solver chosen at capture time
};
static_assert(sizeof(LoopKey) <= sizeof(mpcx_ctx::loop_key), "loop_key too small");

// the bytes of *src, or the zeros already there for a stage that is off
template <class T> static void key_put(T &dst, const T *src) { if (src) memcpy(&dst, src, sizeof dst); }

}  // namespace mpcx
using mpcx::LoopArgs;
using mpcx::LoopStages;

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

// the counting sort of the work queue rides in the kernels of the step (the slot of an agent has 24 bits)
static bool binned(int32_t P) { return P < (1 << 24); }

// The stage set of a run from what the caller passed; refused before anything is launched, whatever n_steps is.
static int32_t check_stages(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const LoopArgs &a, LoopStages *st) {
    if (a.opts && a.opts->stop_mode != MPCX_STOP_CUT) {
        if (a.opts->stop_mode != MPCX_STOP_SPEED)
            return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: unknown stop mode %d (MPCX_STOP_CUT or MPCX_STOP_SPEED)", a.opts->stop_mode);
        if (!std::isfinite(a.opts->v_ref)) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: MPCX_STOP_SPEED with a speed reference v_ref that is not finite");
        if (!a.opts->prev_len) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: MPCX_STOP_SPEED needs prev_len (P zero-initialised int32)");
        st->opts.stop_mode = MPCX_STOP_SPEED; st->opts.v_ref = a.opts->v_ref; st->opts.prev_len = a.opts->prev_len;
    }
    int32_t rc = MPCX_OK;
    if (!mpcx_record_absent(a.log)) st->log = a.log;
    if (st->log && (rc = mpcx_record_validate(ctx, st->log, c->obs_skip)) != MPCX_OK) return rc;
    if (!mpcx_retire_absent(a.retire)) st->retire = a.retire;
    if (st->retire && (rc = mpcx_retire_validate(ctx, st->retire, c->P)) != MPCX_OK) return rc;
    if (!mpcx_scene_absent(a.scene)) {
        st->scene = a.scene;
        const bool traffic = c->n_actors > 0;
        const size_t rows = traffic ? (size_t)(c->pool_rows > 0 ? c->pool_rows : 0) : (size_t)c->P;
        rc = mpcx_scene_validate(ctx, st->scene, st->retire, c->exchange, rows, c->obs_skip);
        if (rc == MPCX_OK && c->P > 0) rc = mpcx_loop_check_rows(ctx, c->P, c->obs_skip, st->scene->n_rows, "scene");
        if (rc != MPCX_OK) return rc;
    }
    if (!mpcx_admit_absent(a.admit)) st->admit = a.admit;
    if (st->admit && (rc = mpcx_admit_validate(ctx, st->admit, st->retire, st->scene, c->exchange)) != MPCX_OK) return rc;
    if (!mpcx_respawn_absent(a.respawn)) st->respawn = a.respawn;
    if (st->respawn && (rc = mpcx_respawn_validate(ctx, st->respawn, st->admit)) != MPCX_OK) return rc;
    if (!mpcx_routes_absent(a.routes)) {
        st->routes = a.routes;
        // (the longest route the conflict search handles is its launch's capacity)
        rc = mpcx_routes_validate(ctx, st->routes, st->respawn, c->path_off, c->path_len, mpcx_interaction_capacity(ip));
        if (rc != MPCX_OK) return rc;
    }
    if (!mpcx_precedence_absent(a.precedence)) st->precedence = a.precedence;
    if (st->precedence && (rc = mpcx_precedence_validate(ctx, st->precedence, st->scene, st->admit)) != MPCX_OK) return rc;
    if (!mpcx_signals_absent(a.signals)) st->signals = a.signals;
    if (ctx->have_braking) {        // in front of the holds' own checks: what the stage cannot run with is refused in its name
        rc = mpcx_braking_validate(ctx, &ctx->braking, c->dl, c->exchange, ctx->lin_passes,
                                   st->signals || !mpcx_actuation_absent(a.actuation) || !mpcx_reservation_absent(a.reservation) || ctx->have_priority || ctx->have_stopsign);
        if (rc != MPCX_OK) return rc;
        st->brake = &ctx->braking;
    }
    if (ctx->have_keepclear) {      // in front of the hold's own checks, so that what the stage cannot run with is refused in its name; it
                                    // reads the signals' pointers and counts only, which the hold's check below then goes through
        rc = mpcx_keepclear_validate(ctx, &ctx->keepclear, st->signals, c->P, c->exchange, !mpcx_reservation_absent(a.reservation));
        if (rc != MPCX_OK) return rc;
        st->keepclear = &ctx->keepclear;
    }
    if (ctx->have_priority) {       // in front of the holds' own checks too: a junction is run by lights, by a manager, or by priority
        rc = mpcx_priority_validate(ctx, &ctx->priority, c->P, c->exchange,
                                    st->signals || !mpcx_actuation_absent(a.actuation) || !mpcx_reservation_absent(a.reservation));
        if (rc != MPCX_OK) return rc;
        st->priority = &ctx->priority;
    }
    if (ctx->have_stopsign) {       // in front of the holds' own checks too: ... or by signs
        rc = mpcx_stopsign_validate(ctx, &ctx->stopsign, c->P, c->exchange,
                                    st->signals                               ? "signals" :
                                    !mpcx_actuation_absent(a.actuation)       ? "actuation" :
                                    !mpcx_reservation_absent(a.reservation)   ? "a reservation" :
                                    ctx->have_priority                        ? "the priority road" : nullptr);
        if (rc != MPCX_OK) return rc;
        st->stopsign = &ctx->stopsign;
    }
    if (!mpcx_reservation_absent(a.reservation)) {  // checks the signals it draws on too, and refuses a controller or advice beside it
        rc = mpcx_reservation_validate(ctx, a.reservation, st->signals, c->P, c->exchange, !mpcx_actuation_absent(a.actuation),
                                       !mpcx_advice_absent(a.advice));
        if (rc != MPCX_OK) return rc;
        st->reserve = a.reservation;
    } else if (!mpcx_actuation_absent(a.actuation)) {      // checks the signals it draws on too
        rc = mpcx_actuation_validate(ctx, a.actuation, st->signals, c->P, c->exchange);
        if (rc != MPCX_OK) return rc;
        mpcx_actuation &act = st->actuation;
        act.phase_groups = a.actuation->phase_groups; act.phase_time = a.actuation->phase_time; act.ctrl_time = a.actuation->ctrl_time;
        act.ctrl_of = a.actuation->ctrl_of; act.jstate = a.actuation->jstate; act.lights = a.actuation->lights; act.calls = a.actuation->calls;
        act.n_per = a.actuation->n_per; act.n_junctions = a.actuation->n_junctions; act.n_phases = a.actuation->n_phases;
        act.n_ctrl = a.actuation->n_ctrl;
        st->actuated = true;
    } else if (st->signals) {
        rc = mpcx_signals_validate(ctx, st->signals, c->exchange);
    }
    if (rc != MPCX_OK) return rc;
    if (!mpcx_advice_absent(a.advice)) {            // (the signals it draws on are checked above)
        rc = mpcx_advise_validate(ctx, a.advice, st->signals, st->actuated, st->speed(), c->P);
        if (rc == MPCX_OK) st->advice = a.advice;
    }
    if (rc != MPCX_OK) return rc;
    if (!mpcx_intent_absent(a.intent)) {
        const int32_t rows = c->n_actors > 0 ? c->pool_rows : c->P;
        rc = mpcx_intent_validate(ctx, a.intent, c->P, c->exchange, c->obs6 ? rows : 0, c->obs_skip);
        if (rc == MPCX_OK) st->intent = a.intent;
    }
    if (rc != MPCX_OK) return rc;
    if (ctx->have_following) {
        rc = mpcx_following_validate(ctx, &ctx->following, c->P, c->exchange);
        if (rc == MPCX_OK) st->follow = &ctx->following;
    }
    if (rc != MPCX_OK) return rc;
    if (ctx->have_safety) {
        if (!c->obs_skip) return mpcx_fail(ctx, MPCX_E_INVALID, "safety: the descriptor has no obs_skip (the agents' own pool rows)");
        rc = mpcx_safety_validate(ctx, &ctx->safety, ip, c->P, c->n_actors > 0 ? c->pool_rows : c->P, c->exchange);
        if (rc == MPCX_OK) st->safety = &ctx->safety;
    }
    if (rc != MPCX_OK) return rc;
    if (ctx->have_sight) {
        if (!st->retire || !st->scene)
            return mpcx_fail(ctx, MPCX_E_INVALID, "sight: the run has no retirement and scene (the conflict search's list of present rows is the scene's)");
        // (the scene has been checked: the layout is not agent-sharded and the descriptor has obs_skip)
        rc = mpcx_sight_validate(ctx, &ctx->sight, c->P, c->n_actors > 0 ? c->pool_rows : c->P);
        if (rc == MPCX_OK) st->sight = &ctx->sight;
    }
    if (rc == MPCX_OK && st->brake) {       // the stop lines and the hold words of the stages that are on in this run
        st->lines.path_stop = st->signals ? st->signals->path_stop : st->priority ? st->priority->path_stop : st->stopsign->path_stop;
        st->lines.n_points = st->signals ? st->signals->n_points : st->priority ? st->priority->n_points : st->stopsign->n_points;
        st->lines.held = st->signals ? st->signals->held : nullptr;
        st->lines.boxed = st->keepclear ? st->keepclear->boxed : nullptr;
        // (the priority road and stop signs never run together: the mark launch reads the one's yielding or the other's stopping in the same slot)
        st->lines.yielding = st->priority ? st->priority->yielding : st->stopsign ? st->stopsign->stopping : nullptr;
    }
    return rc;
}

// The middle of a step, the same on both paths: (the sight stage ->) the conflict search (-> the safety stage) (-> the signal stage) (-> the keep-clear stage) (-> the priority or stop-sign stage) (-> the following stage) (-> the firm hold's mark) -> lin_passes x (reference
// window (-> the advice stage) (-> the following clamp) (-> the firm hold's clamp) -> solve).
// ix: what the caller knows about the pool (who packs and predicts its rows, where the agents and the scripted cars sit); the rest is filled
// in here.  rollout_done: xbar is written already, in stream order (head_kernel); else the first pass joins the rollout the caller forked.
static int32_t enqueue_search_and_solve(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const LoopStages &st,
                                        mpcx_interaction_extras ix, int32_t pool_rows, bool rollout_done) {
    const int P = c->P;
    const bool speed = st.speed(), bins = binned(P);
    const int32_t *done = st.done();
    int32_t *queue_len = st.retire ? ctx->ticket + MPCX_TICKET_QUEUE_LEN : nullptr;
    // the conflict search leaves the cut lengths of the previous step in ctx->prev_cut (the queue of the QP kernel puts the agents whose
    // cut moved at the front) and files every agent under its work-queue key (previous iteration count + "the cut moved"): hard problems first.  The window
    // selection then writes the queue order and the plant kernel resets bins and ticket, so the counting sort costs no launch of its own.
    ix.prev_save = ctx->prev_cut;
    ix.near = near_hints(ctx, P);
    ix.bin_hint = bins ? c->iters : nullptr;
    ix.done = done;
    ix.absent = st.scene ? st.scene->absent : nullptr;
    if (st.precedence) { ix.prec = st.precedence->prec; ix.stand = st.precedence->stand; }
    ix.sight = st.sight;
    if (speed) ix.key_prev = c->cut_len;        // "the cut moved" = the stop index moved
    int32_t rc = mpcx_interaction_enqueue(ctx, ip, P, c->state, c->path_xyyaw, c->path_cs, c->path_off, c->path_len,
                                          speed ? st.opts.prev_len : c->cut_len /* previous step's cut; read before it is rewritten */, pool_rows,
                                          c->obs6, c->obs_off, c->obs_cnt, c->obs_skip, c->traj_idx, c->hit_idx, c->hit_xy, c->cut_len, ix);
    if (rc != MPCX_OK) return rc;
    if (st.safety) {
        rc = mpcx_safety_enqueue(ctx, ip, P, c->state, c->path_off, c->traj_idx, done, pool_rows, c->obs6, ctx->pred, c->obs_off, c->obs_cnt,
                                 c->obs_skip, ix.absent, st.safety);
        if (rc != MPCX_OK) return rc;
    }
    if (st.signals) {
        rc = st.reserve  ? mpcx_reserve_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.signals, st.reserve)
           : st.actuated ? mpcx_actuated_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.signals, &st.actuation)
                         : mpcx_signal_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.signals);
        if (rc != MPCX_OK) return rc;
    }
    if (st.keepclear) {
        rc = mpcx_keepclear_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.signals, st.keepclear);
        if (rc != MPCX_OK) return rc;
    }
    if (st.priority) {
        rc = mpcx_priority_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.priority);
        if (rc != MPCX_OK) return rc;
    }
    if (st.stopsign) {
        rc = mpcx_stopsign_enqueue(ctx, P, c->dl, c->state, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.stopsign);
        if (rc != MPCX_OK) return rc;
    }
    if (st.follow) {
        rc = mpcx_follow_enqueue(ctx, P, c->dl, speed, c->state, c->path_xyyaw, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, pool_rows,
                                 c->obs6, c->obs_off, c->obs_cnt, c->obs_skip, ix.absent, st.follow);
        if (rc != MPCX_OK) return rc;
    }
    if (st.brake) {
        rc = mpcx_brake_mark_enqueue(ctx, P, c->dl, speed, c->path_off, c->path_len, c->traj_idx, c->target_ind, ctx->win_len, done, st.lines.path_stop,
                                     st.lines.n_points, st.lines.held, st.lines.boxed, st.lines.yielding, st.brake);
        if (rc != MPCX_OK) return rc;
    }
    const bool firm = st.brake && speed;        // the window stage reads the mark's lengths
    // lib/mpc.py:226-237: MAX_ITER passes of (reference window, rollout, QP); from the second pass on the window is spaced by the
    // previous pass's speeds (row 2 of its x) and the rollout uses its inputs.  (Where a pass fails the reference crashes in the next
    // one -- zip over None; here the next pass starts from the untouched warm start, as after a failed step.)
    const int Wd = ctx->mpc.T + 1;
    for (int pass = 0; pass < ctx->lin_passes; pass++) {
        const bool first = pass == 0;
        // the first pass writes the queue order and joins the rollout of this step; a later one forks its own
        mpcx_window_extras wx{bins && first, near_hints(ctx, P), c->traj_idx, first};
        wx.rollout_done = rollout_done;
        if (speed) { wx.stop_idx = c->cut_len; wx.v_ref = st.opts.v_ref; wx.len_seen = st.opts.prev_len; }
        wx.done = done; wx.queue_len = queue_len;
        rc = mpcx_window_enqueue(ctx, P, c->state, c->u_sol, c->path_xyyaw, c->path_v, c->path_off, firm ? ctx->win_len : speed ? c->path_len : c->cut_len, c->dl,
                                 c->target_ind, pass ? c->x_sol + 2 * Wd : nullptr, 4 * (int64_t)Wd, c->xref, c->reaches_end, c->xbar, wx);
        if (rc != MPCX_OK) return rc;
        if (st.advice) {
            rc = mpcx_advise_enqueue(ctx, P, c->dl, c->path_off, c->path_len, c->traj_idx, c->cut_len, done, st.signals, st.advice, c->xref);
            if (rc != MPCX_OK) return rc;
        }
        if (st.follow && speed) {
            rc = mpcx_follow_cap_enqueue(ctx, P, done, st.follow, c->xref);
            if (rc != MPCX_OK) return rc;
        }
        if (firm) {
            rc = mpcx_brake_clamp_enqueue(ctx, P, c->dl, c->state, c->path_xyyaw, c->path_off, c->path_len, c->traj_idx, st.opts.prev_len, done,
                                          st.lines.path_stop, st.lines.n_points, st.brake, c->xref);
            if (rc != MPCX_OK) return rc;
        }
        // (further linearisation passes build their order in line, from the iteration counts of the pass before)
        const mpcx_qp_order ord{bins && first, c->iters, c->cut_len, ctx->prev_cut, queue_len};
        rc = mpcx_qp_enqueue(ctx, P, c->state, c->xref, c->xbar, c->reaches_end, c->u_sol, c->x_sol, c->u_sol, c->status, c->iters, c->kkt, ord);
        if (rc != MPCX_OK) return rc;
    }
    return MPCX_OK;
}

// the plant update in a launch of its own; it leaves the queue bins and the ticket zeroed for the next step
static int32_t enqueue_plant(mpcx_ctx *ctx, const mpcx_closed_loop *c, const int32_t *done) {
    const mpcx_plant_extras px{c->iters, binned(c->P), done};
    const int32_t rc = mpcx_plant_enqueue(ctx, c->P, c->state, c->u_sol, c->status, c->applied, px);
    if (rc == MPCX_OK) ctx->bins_clean = binned(c->P);
    return rc;
}

static int32_t enqueue_step(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const LoopStages &st) {
    const int P = c->P;
    const bool speed = st.speed();
    ctx->bins_clean = false;        // until the plant kernel of this step is enqueued
    int32_t rc, pool_rows = P;
    if (st.admit) {
        const int32_t na = c->n_actors > 0 ? c->n_actors : 0;
        rc = mpcx_admit_enqueue(ctx, ip, P, c->state, c->obs_off, c->obs_cnt, c->obs_skip, st.retire->done, st.scene->n_rows, st.scene->absent, na,
                                c->actors, c->actor_state, c->tape, c->tape_rows, c->actor_row, st.admit);
        if (rc != MPCX_OK) return rc;
        if (st.precedence && st.precedence->mode == MPCX_PRECEDENCE_ENTRY) {
            rc = mpcx_precedence_enqueue(ctx, P, c->obs_off, c->obs_skip, st.admit, st.precedence);
            if (rc != MPCX_OK) return rc;
        }
    }
    // the warm-start rollout of this step needs only the states and the previous solution: it runs on the side stream BESIDE the pool pack,
    // the prediction and the conflict search (a chain of T dependent sincos / tan per agent, 35-45 us) and is joined by the window selection
    rc = mpcx_rollout_fork(ctx, P, c->state, c->u_sol, c->xbar, st.done());
    if (rc != MPCX_OK) return rc;
    mpcx_interaction_extras ix;
    mpcx_intent_launch plans;
    if (st.intent) {        // the previous step's solution and its status, as they stand at the head of this step
        plans.u_sol = c->u_sol; plans.status = c->status; plans.done = st.done(); plans.absent = st.scene ? st.scene->absent : nullptr;
        plans.in = *st.intent;
        ix.intent = &plans;
    }
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
    rc = enqueue_search_and_solve(ctx, ip, c, st, ix, pool_rows, false);
    if (rc != MPCX_OK) return rc;
    rc = enqueue_plant(ctx, c, st.done());
    if (rc != MPCX_OK) return rc;
    if (st.log) {
        rc = mpcx_record_enqueue(ctx, ip, P, c->state, c->applied, c->x_sol, c->path_xyyaw, c->path_off, c->path_len, c->target_ind, c->cut_len,
                                 c->traj_idx, c->hit_idx, c->status, c->iters, pool_rows, c->obs6, c->obs_off, c->obs_cnt, c->obs_skip, st.log,
                                 speed ? c->path_len : nullptr, st.done(), st.scene ? st.scene->absent : nullptr);
        if (rc != MPCX_OK) return rc;
    }
    // the goal test of the record stage (len(cx) = cut_len, the whole path in speed mode)
    if (st.retire) rc = mpcx_retire_enqueue(ctx, P, c->state, c->applied, c->path_xyyaw, c->path_off, c->path_len, c->target_ind,
                                            speed ? c->path_len : c->cut_len, st.retire, st.scene, c->obs_skip);
    if (rc != MPCX_OK) return rc;
    if (st.respawn && st.routes)
        rc = mpcx_route_enqueue(ctx, P, c->state, c->applied, c->u_sol, c->traj_idx, c->target_ind, c->cut_len, c->iters,
                                speed ? st.opts.prev_len : nullptr, c->obs_skip, st.scene->n_rows, st.log, st.retire, st.admit, st.respawn, st.routes);
    else if (st.respawn)
        rc = mpcx_respawn_enqueue(ctx, P, c->state, c->applied, c->u_sol, c->traj_idx, c->target_ind, c->cut_len, c->iters,
                                  speed ? st.opts.prev_len : nullptr, c->obs_skip, st.scene->n_rows, st.log, st.retire, st.admit, st.respawn);
    return rc;
}

// A run of n_steps with step fusion (mpcx_set_step_fusion; closed_loop_run decides where it applies: the local pool, no scripted traffic, one
// linearisation pass, no optional stage): per step ONE launch for what belongs to an agent alone -- the plant update of the step before
// (from the second step of the run on), the pack and prediction of its pool row, its warm-start rollout -- then the middle of a step as
// enqueue_step has it; the last step's plant update ends the run in a launch of its own.  Nothing runs on the side stream and neither
// event is touched.  The buffers hold the bits enqueue_step leaves.
static int32_t enqueue_fused_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const LoopStages &st,
                                 int32_t n_steps) {
    const int P = c->P;
    for (int s = 0; s < n_steps; s++) {
        ctx->bins_clean = false;        // until the plant update of this step is enqueued
        int32_t rc = mpcx_head_enqueue(ctx, ip, P, c->state, c->applied, c->u_sol, c->status, c->iters, c->xbar, c->obs6, s > 0, binned(P));
        if (rc != MPCX_OK) return rc;
        mpcx_interaction_extras ix;
        ix.pack_state = c->state; ix.pack_applied = c->applied;
        ix.predicted = true;
        rc = enqueue_search_and_solve(ctx, ip, c, st, ix, P, true);
        if (rc != MPCX_OK) return rc;
    }
    return enqueue_plant(ctx, c, nullptr);
}

static int32_t closed_loop_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c, const LoopArgs &args,
                               int32_t n_steps, int32_t use_graph) {
    if (!ctx) return MPCX_E_INVALID;
    if (!ctx->have_mpc) return mpcx_fail(ctx, MPCX_E_INVALID, "mpcx_set_mpc_params has not been called");
    if (!ip || !c || n_steps < 0 || c->P < 0) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: null descriptor or negative count");
    LoopStages st;
    int32_t rc = check_stages(ctx, ip, c, args, &st);
    if (rc != MPCX_OK) return rc;
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
    rc = mpcx_ensure_pred(ctx, pool_rows * ip->pred_steps * 4);
    if (rc != MPCX_OK) return rc;
    if (c->n_actors > 0) {
        rc = mpcx_traffic_validate(ctx, c->n_actors, c->actors, c->tape, c->tape_rows, c->actor_row, c->pool_rows);
        if (rc != MPCX_OK) return rc;
        rc = mpcx_loop_check_rows(ctx, c->P, c->ego_row, c->pool_rows);
        if (rc != MPCX_OK) return rc;
    }
    rc = mpcx_ensure_ticket(ctx);
    if (rc != MPCX_OK) return rc;
    if (st.admit) {
        rc = mpcx_admit_prepare(ctx, (size_t)st.scene->n_rows);
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
    if (st.brake) {
        rc = mpcx_grow(ctx, (void **)&ctx->win_len, &ctx->win_len_cap, (size_t)c->P * sizeof(int32_t), "the window lengths");
        if (rc != MPCX_OK) return rc;
    }

    if (!use_graph) {
        if (ctx->step_fusion && c->exchange == 0 && c->n_actors == 0 && ctx->lin_passes == 1 && st.none())
            return enqueue_fused_run(ctx, ip, c, st, n_steps);
        for (int s = 0; s < n_steps; s++) {
            rc = enqueue_step(ctx, ip, c, st);
            if (rc != MPCX_OK) return rc;
        }
        return MPCX_OK;
    }

    if (!ctx->stream) return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: graph replay needs a non-default stream");
    if (ctx->prof_qp)       // the event pairs of mpcx_profile_qp cannot be recorded inside a replayed graph: say so instead of reporting 0 launches
        return mpcx_fail(ctx, MPCX_E_INVALID, "closed_loop_run: mpcx_profile_qp is on; the QP launches of a replayed graph are not bracketed by events -- run without graph or switch the hook off");
    mpcx::LoopKey key;
    memset(&key, 0, sizeof key);
    using mpcx::key_put;
    key_put(key.desc, c); key_put(key.ip, ip); key_put(key.mpc, &ctx->mpc);
    key_put(key.log, st.log); key_put(key.retire, st.retire); key_put(key.scene, st.scene); key_put(key.admit, st.admit);
    key_put(key.respawn, st.respawn); key_put(key.routes, st.routes); key_put(key.precedence, st.precedence); key_put(key.signals, st.signals);
    key_put(key.advice, st.advice); key_put(key.intent, st.intent); key_put(key.reservation, st.reserve);
    key_put(key.following, st.follow);
    key_put(key.safety, st.safety);
    key_put(key.sight, st.sight);
    key_put(key.keepclear, st.keepclear);
    key_put(key.priority, st.priority);
    key_put(key.stopsign, st.stopsign);
    key_put(key.braking, st.brake);
    key.opts = st.opts; key.actuation = st.actuation;
    key.admit_tab = ctx->admit_tab; key.pred = ctx->pred; key.tune = ctx->tune; key.order = ctx->order;
    key.prev_cut = ctx->prev_cut; key.bins = ctx->bins; key.stats = ctx->stats; key.win_len = st.brake ? ctx->win_len : nullptr;
    key.qp_solver = ctx->qp_solver; key.lin_passes = ctx->lin_passes; key.qp_plain_rounds = ctx->qp_plain_rounds ? 1 : 0;
    if (!ctx->loop_exec || memcmp(&key, ctx->loop_key, sizeof key) != 0) {
        if (ctx->loop_exec) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipGraphExecDestroy(ctx->loop_exec);
            ctx->loop_exec = nullptr;
        }
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipStreamBeginCapture failed");
        rc = enqueue_step(ctx, ip, c, st);
        hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
        if (rc != MPCX_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess || !graph) return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: stream capture failed: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&ctx->loop_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { ctx->loop_exec = nullptr; return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipGraphInstantiate: %s", hipGetErrorString(e)); }
        memcpy(ctx->loop_key, &key, sizeof key);
    }
    for (int s = 0; s < n_steps; s++)
        if (hipGraphLaunch(ctx->loop_exec, ctx->stream) != hipSuccess)
            return mpcx_fail(ctx, MPCX_E_LAUNCH, "closed_loop_run: hipGraphLaunch failed");
    return MPCX_OK;
}

// The entry points: each names the stages it has parameters for, in LoopArgs' order; the rest are off.

extern "C" int32_t mpcx_closed_loop_run(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                        int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_logged(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_opts(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                             const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_retire(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                               int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_scene(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                              const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                              const mpcx_scene *scene, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_admit(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                              const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                              const mpcx_scene *scene, const mpcx_admit *admit, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_respawn(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_routes(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                               const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                               const mpcx_routes *routes, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_precedence(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                   const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                   const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                   const mpcx_routes *routes, const mpcx_precedence *precedence, int32_t n_steps,
                                                   int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes, precedence}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_signals(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                                int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes, precedence, signals}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_actuated(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                 const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                 const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                 const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                                 const mpcx_actuation *actuation, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes, precedence, signals, actuation}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_advised(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                                const mpcx_actuation *actuation, const mpcx_advice *advice, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes, precedence, signals, actuation, advice}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_intent(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                               const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                               const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                               const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                               const mpcx_actuation *actuation, const mpcx_advice *advice, const mpcx_intent *intent,
                                               int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes, precedence, signals, actuation, advice, intent}, n_steps, use_graph);
}
extern "C" int32_t mpcx_closed_loop_run_reserved(mpcx_ctx *ctx, const mpcx_interaction_params *ip, const mpcx_closed_loop *c,
                                                 const mpcx_run_log *log, const mpcx_closed_loop_opts *opts, const mpcx_retire *retire,
                                                 const mpcx_scene *scene, const mpcx_admit *admit, const mpcx_respawn *respawn,
                                                 const mpcx_routes *routes, const mpcx_precedence *precedence, const mpcx_signals *signals,
                                                 const mpcx_actuation *actuation, const mpcx_advice *advice, const mpcx_intent *intent,
                                                 const mpcx_reservation *reservation, int32_t n_steps, int32_t use_graph) {
    return closed_loop_run(ctx, ip, c, {log, opts, retire, scene, admit, respawn, routes, precedence, signals, actuation, advice, intent, reservation},
                           n_steps, use_graph);
}
