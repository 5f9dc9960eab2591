// mpcx_common.h -- shared device helpers for the libmpcx.so kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mpcx.h"
#include "mpcx_qp_consts.h"
#include <vector>

struct mpcx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    mpcx_mpc_params mpc = {};
    bool have_mpc = false;
    int32_t *ticket = nullptr;  // device words: [0] work-queue head of the persistent QP kernel, [4] the list of problems the condensed solver gives up on, [5] the head of the launch that works that list off, [6] the length of the step's queue under retirement; 8 allocated
    int n_cu = 0;               // compute units of the device
    // device scratch that grows on demand (mpcx_grow); every capacity is in bytes
    double *pred = nullptr;     // predicted obstacle disc centres [NOBS][steps][2 discs][2]
    size_t pred_cap = 0;
    hipGraphExec_t loop_exec = nullptr;   // cached one-step graph of mpcx_closed_loop_run (nullptr = none)
    unsigned char loop_key[2160] = {};    // what the cached graph was captured for: an mpcx::LoopKey (mpcx_loop.hip, which checks that it fits)
    const mpcx_qp_tuning *tune = nullptr; // per-instance tuning rows (device) or nullptr
    int32_t tune_rows = 0;
    mpcx_following following = {};        // car following (mpcx_set_following): the struct by value, padding zeroed; all zeros while off
    bool have_following = false;
    mpcx_safety safety = {};              // the near-miss log (mpcx_set_safety): the struct by value, padding zeroed; all zeros while off
    bool have_safety = false;
    mpcx_sight sight = {};                // line of sight (mpcx_set_sight): the struct by value, padding zeroed; all zeros while off
    bool have_sight = false;
    struct SightTables {                  // the offset tables of a mpcx_sight that were read back and passed their check (mpcx_sight_validate)
        const int32_t *set_off = nullptr, *hp_off = nullptr;
        const double *hp = nullptr;
        int32_t n_sets = 0, n_occ = 0;
        bool ok = false;
    } sight_tables;
    mpcx_keepclear keepclear = {};        // keep clear (mpcx_set_keepclear): the struct by value, padding zeroed; all zeros while off
    bool have_keepclear = false;
    struct KeepClearTable {               // the conflict table of a mpcx_keepclear that was read back and passed its check (mpcx_keepclear_validate)
        const int32_t *conflict = nullptr;
        int32_t n_moves = 0;
        bool ok = false;
    } keepclear_table;
    mpcx_priority priority = {};          // priority road (mpcx_set_priority): the struct by value (it has no padding); all zeros while off
    bool have_priority = false;
    struct PriorityTables {               // the per-movement tables of a mpcx_priority that were read back and passed their check (mpcx_priority_validate)
        const int32_t *conflict = nullptr, *rank = nullptr;
        const double *gap = nullptr;
        int32_t n_moves = 0;
        bool ok = false;
    } priority_tables;
    mpcx_stopsign stopsign = {};          // stop signs (mpcx_set_stopsign): the struct by value (it has no padding); all zeros while off
    bool have_stopsign = false;
    struct StopSignTables {               // the per-movement tables of a mpcx_stopsign that were read back and passed their check (mpcx_stopsign_validate)
        const int32_t *conflict = nullptr, *lane = nullptr, *sign = nullptr;
        const double *gap = nullptr;
        int32_t n_moves = 0;
        bool ok = false;
    } stopsign_tables;
    mpcx_braking braking = {};            // firm hold (mpcx_set_braking): the struct by value (it has no padding); all zeros while off
    bool have_braking = false;
    int32_t *win_len = nullptr;           // scratch of mpcx_closed_loop_run with the firm hold on: [P] the lengths the window stage is handed in place of path_len
    size_t win_len_cap = 0;
    const int32_t *order_hint = nullptr;  // iteration counts of a previous solve (device) or nullptr (mpcx_qp_set_order_hint)
    const int32_t *order_now = nullptr, *order_prev = nullptr;   // optional pair: entries that differ mark a discontinuous change of the reference
    // scratch of mpcx_closed_loop_run for P agents: [P] cut lengths of the previous step | [3 P] what the conflict search's nearest-index
    // scan found, for the window selection (mpcx_window_extras::near)
    int32_t *prev_cut = nullptr;
    size_t prev_cut_cap = 0;
    int32_t *order = nullptr;   // scratch: work-queue order built from the hint | per-block key histograms | list of given-up problems | 2 counters
    size_t order_cap = 0;
    // closed loop: the counting sort of the work queue rides in the kernels of the step instead of two launches and two fills of its own.
    // The conflict search files every agent under its queue key (bins[key]++ -> slot), the window selection turns (key, slot) into the
    // agent's place in `order`, the plant kernel zeroes the bins and the ticket for the next step.
    int32_t *bins = nullptr;    // [MPCX_ORDER_COPIES][MPCX_ORDER_BINS] counters (agent p counts in copy p % COPIES: 32 k atomics on 64 words are slow) | [P] (key << 24 | slot)
    size_t bins_cap = 0;
    bool bins_clean = false;    // host's knowledge: the counters and the ticket are zero (the last closed-loop step ran through and nothing has drawn tickets since)
    hipStream_t side = nullptr; // side stream of mpcx_mpc_prepare_batch: the warm-start rollout runs beside the window selection (fork / join by events)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    double *cs = nullptr;       // scratch of mpcx_expand_batch: (cos, sin) of the nodes' headings
    size_t cs_cap = 0;
    void *multi = nullptr;      // scratch of mpcx_expand_multi_batch and mpcx_astar_batch (segment descriptors + block tables)
    size_t multi_cap = 0;
    int qp_solver = 0;          // 0 = automatic, 1 = condensed (one wavefront per QP), 2 = stage-structured (mpcx_set_qp_solver)
    bool step_fusion = true;    // mpcx_closed_loop_run takes plant, prediction and rollout in one launch where it can (mpcx_set_step_fusion)
    bool qp_plain_rounds = true;        // the stage solver runs the plain copies of its row passes where a round allows it (mpcx_qp_set_plain_rounds)
    int lin_passes = 1;         // linearisation passes per step of mpcx_closed_loop_run (lib/mpc.py MAX_ITER; mpcx_set_linearisation_passes)
    bool prof_qp = false;       // bracket qp_kernel launches with events (mpcx_profile_qp)
    std::vector<hipEvent_t> prof_ev;   // start/stop pairs recorded so far
    std::vector<hipEvent_t> prof_free; // recycled events
    unsigned long long *stats = nullptr;    // run statistics of mpcx_closed_loop_run: per wavefront of the plant kernel (agent-steps, iterations, failures, max iterations)
    size_t stats_slots = 0;                 // wavefront slots allocated
    void *comm = nullptr;       // ncclComm_t (mpcx_comm_init) or nullptr = single rank
    int comm_world = 1, comm_rank = 0;
    double *xchg = nullptr;     // all-gather landing buffer of the agent-sharded layout
    size_t xchg_cap = 0;
    double *admit_tab = nullptr;    // table of the admission stage (mpcx_admit.hip): [pool rows][3] poses | [pool rows] int32 tags
    size_t admit_tab_cap = 0;
    char err[256] = {};
};

// The stages of a step.  Each is the whole of the C entry point of the same name (checks included) plus one struct of what only
// mpcx_closed_loop_run passes: default-constructed = the stand-alone call.
// what the shared-plans launch reads beside the conflict search's own arguments (state, obs_skip, the pool and its prediction)
struct mpcx_intent_launch {
    const double *u_sol = nullptr;      // P x 2 x T, the previous step's solution
    const int32_t *status = nullptr;    // P, of that solution
    const int32_t *done = nullptr;      // P or nullptr
    const int32_t *absent = nullptr;    // pool rows or nullptr
    mpcx_intent in = {};
};
struct mpcx_interaction_extras {
    // local pool: the prediction kernel packs the pool rows from the agents' states and applied inputs itself (no launch of its own)
    const double *pack_state = nullptr, *pack_applied = nullptr;
    bool predicted = false;             // the pool rows are packed and predicted already, in stream order (head_kernel): no prediction launch
    // ... with scripted traffic in the pool: agent q is packed into row ego_row[q], and the n_actors rows actor_row[] (written by
    // traffic_kernel just before) are predicted as they stand; nullptr: row q is agent q
    const int32_t *ego_row = nullptr, *actor_row = nullptr;
    int32_t n_ego = 0, n_actors = 0;
    int32_t *prev_save = nullptr;       // where the cut lengths as read are left (the queue order's `moved` test)
    // speed-reference mode: prev_cut_len is the previous PATH length there and cut_len holds the stop index, so the `moved` test and
    // prev_save read the previous stop index from here (the cut_len buffer itself, before it is rewritten); nullptr: prev_cut_len
    const int32_t *key_prev = nullptr;
    // the conflict search and the window selection both run calc_nearest_index_in_direction for the same agent, state and path, mostly
    // from the same start index.  The conflict search leaves (its start index, the largest, the smallest of its three nearest indices
    // or -1) here, 3 ints per agent, and the window selection takes the conflict search's answer where that is provably its own.
    int32_t *near = nullptr;
    const int32_t *bin_hint = nullptr;  // iteration counts of the previous step: every agent is filed in ctx->bins under its queue key
    const int32_t *done = nullptr;      // retirement (mpcx_retire::done): an agent with done[p] != 0 is not searched, not filed and none of its outputs is written
    // departure (mpcx_scene::absent, n_obs_pool words; needs done): pool rows with absent[r] != 0 are neither predicted nor in anybody's obstacle list
    const int32_t *absent = nullptr;
    // right of way (mpcx_precedence::prec / stand, n_obs_pool words / rows of four doubles; needs absent): the prediction also stores every
    // predicted row's standing record, and an agent sees the present rows whose word is larger than its own row's through that record
    const int32_t *prec = nullptr;
    double *stand = nullptr;
    // shared plans (mpcx_intent.hip; nullptr: off): one more launch between the prediction and the conflict search re-rolls the plans of the
    // sharing agents into their own pool rows
    const mpcx_intent_launch *intent = nullptr;
    // line of sight (mpcx_sight.hip; nullptr: off; needs absent): one more launch behind the prediction and the intent stage writes every
    // agent's word of seen rows, and the conflict search takes its SIGHT instantiation (mpcx_interaction_sight.hip)
    const mpcx_sight *sight = nullptr;
};
struct mpcx_window_extras {
    bool scatter = false;               // turn the conflict search's (key, slot) in ctx->bins into the queue order in ctx->order
    const int32_t *near = nullptr, *tidx = nullptr;   // mpcx_interaction_extras::near and the conflict search's updated traj_idx
    bool rollout_forked = false;        // the rollout of this step is in flight on the side stream already (mpcx_rollout_fork)
    bool rollout_done = false;          // ... or xbar is written already, in stream order (head_kernel): nothing is forked and nothing joined
    // mpcx_mpc_prepare_batch_stop: the stop index per agent (nullptr: none, the two below are not read), the speed reference in front of
    // it and where the window kernel leaves the path length it saw
    const int32_t *stop_idx = nullptr;
    double v_ref = 0.0;
    int32_t *len_seen = nullptr;
    // retirement (mpcx_retire::done; needs scatter): a retired agent gets no place in the order and no output; queue_len <- the length of
    // this step's queue (the agents that were filed), which the solve then draws its tickets up to
    const int32_t *done = nullptr;
    int32_t *queue_len = nullptr;
};
struct mpcx_qp_order {                  // where the work-queue order of a solve comes from
    bool ready = false;                 // it is in ctx->order already and the ticket is zero (mpcx_window_extras::scatter)
    const int32_t *hint = nullptr, *now = nullptr, *prev = nullptr;   // else built from these as mpcx_qp_set_order_hint describes; all nullptr: no order
    const int32_t *queue_len = nullptr; // with ready: the order holds *queue_len entries, not B (device word; retirement)
};
struct mpcx_plant_extras {
    const int32_t *stats_iters = nullptr;   // the step's iteration counts: the step feeds the run statistics (ctx->stats)
    bool reset_bins = false;                // zero the queue bins and the ticket for the next step
    const int32_t *done = nullptr;          // retirement: a retired agent's state, applied and u are left alone and it feeds no statistics
};
int32_t mpcx_interaction_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const double *path_xyyaw,
                               const double *path_cs, const int32_t *path_off, const int32_t *path_len, const int32_t *prev_cut_len,
                               int32_t n_obs_pool, const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip,
                               int32_t *traj_idx, int32_t *hit_idx, double *hit_xy, int32_t *cut_len, const mpcx_interaction_extras &x);   // mpcx_interaction.hip
// the path points that launch makes room for: ip->max_path_len (0 = MPCX_MAX_REMAINING; never below 512) rounded up to a multiple of 64
int32_t mpcx_interaction_capacity(const mpcx_interaction_params *ip);                                                                    // mpcx_interaction.hip
int32_t mpcx_window_enqueue(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm, const double *path_xyyaw, const double *path_v,
                          const int32_t *path_off, const int32_t *path_len, double dl, int32_t *target_ind, const double *ov, int64_t ov_stride,
                          double *xref, uint8_t *reaches_end, double *xbar, const mpcx_window_extras &x);                                   // mpcx_prepare.hip
int32_t mpcx_qp_enqueue(mpcx_ctx *ctx, int32_t B, const double *x0, const double *xref, const double *xbar, const uint8_t *reaches_end,
                      const double *u_warm, double *x_out, double *u_out, int32_t *status, int32_t *iters, double *kkt, const mpcx_qp_order &ord);   // mpcx_qp.hip
int32_t mpcx_plant_enqueue(mpcx_ctx *ctx, int32_t B, double *state, double *u, const int32_t *status, double *applied, const mpcx_plant_extras &x);   // mpcx_prepare.hip
int32_t mpcx_head_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, double *state, double *applied, double *u,
                          const int32_t *status, const int32_t *iters, double *xbar, double *obs6, bool plant, bool reset_bins);                   // mpcx_prepare.hip

int32_t mpcx_fail(mpcx_ctx *ctx, int32_t code, const char *fmt, ...);
int32_t mpcx_check_launch(mpcx_ctx *ctx, const char *what);
// grow-on-demand device scratch: *p holds at least need_bytes afterwards (contents are not kept); `what` names it in the error text (mpcx_api.hip)
int32_t mpcx_grow(mpcx_ctx *ctx, void **p, size_t *cap_bytes, size_t need_bytes, const char *what);
int32_t mpcx_ensure_pred(mpcx_ctx *ctx, size_t need_doubles);   // prediction scratch (mpcx_interaction.hip)
// done (retirement): the xbar rows of retired agents are neither computed nor written
int32_t mpcx_rollout_fork(mpcx_ctx *ctx, int32_t B, const double *state, const double *u_warm, double *xbar, const int32_t *done = nullptr);   // mpcx_prepare.hip
int32_t mpcx_traffic_validate(mpcx_ctx *ctx, int32_t n_actors, const mpcx_traffic_actor *actors, const double *tape, int64_t tape_rows,
                              const int32_t *pool_row, int32_t n_obs_pool);                                      // mpcx_traffic.hip
int32_t mpcx_traffic_enqueue(mpcx_ctx *ctx, int32_t n_actors, const mpcx_traffic_actor *actors, double *actor_state, const double *tape,
                             int64_t tape_rows, const int32_t *pool_row, int32_t n_obs_pool, double *obs6);       // mpcx_traffic.hip
// the run log's record stage (mpcx_record.hip): "no log" test, check of the descriptor, the launch alone
bool mpcx_record_absent(const mpcx_run_log *log);
int32_t mpcx_record_validate(mpcx_ctx *ctx, const mpcx_run_log *log, const int32_t *obs_skip);
int32_t mpcx_record_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const double *applied,
                            const double *x_sol, const double *path_xyyaw, const int32_t *path_off, const int32_t *path_len,
                            const int32_t *target_ind, const int32_t *cut_len, const int32_t *traj_idx, const int32_t *hit_idx,
                            const int32_t *status, const int32_t *iters, int32_t n_obs_pool, const double *obs6, const int32_t *obs_off,
                            const int32_t *obs_cnt, const int32_t *obs_skip, const mpcx_run_log *log,
                            const int32_t *goal_len = nullptr,       // goal_len: mpcx_record_step_batch_goal
                            const int32_t *done = nullptr,           // retirement: a retired agent is skipped entirely
                            const int32_t *absent = nullptr);        // departure (mpcx_scene::absent): the clearance skips absent pool rows
// retirement at the goal (mpcx_retire.hip): "no retirement" test, check of the struct, the launch alone
bool mpcx_retire_absent(const mpcx_retire *r);
int32_t mpcx_retire_validate(mpcx_ctx *ctx, const mpcx_retire *r, int32_t P);
int32_t mpcx_retire_enqueue(mpcx_ctx *ctx, int32_t P, const double *state, double *applied, const double *path_xyyaw, const int32_t *path_off,
                            const int32_t *path_len, const int32_t *target_ind, const int32_t *goal_len, const mpcx_retire *r,
                            const mpcx_scene *scene = nullptr, const int32_t *own_row = nullptr);     // departure: absent[own_row[q]] <- 1 on arrival
// departure (mpcx_retire.hip): "no scene" test, check of the struct against the run
bool mpcx_scene_absent(const mpcx_scene *s);
int32_t mpcx_scene_validate(mpcx_ctx *ctx, const mpcx_scene *s, const mpcx_retire *retire, int32_t exchange, size_t pool_rows, const int32_t *obs_skip);
// admission (mpcx_admit.hip): "no admission" test, check of the struct against the run, the table (grown and cleared outside any capture),
// the two launches alone
bool mpcx_admit_absent(const mpcx_admit *a);
int32_t mpcx_admit_validate(mpcx_ctx *ctx, const mpcx_admit *a, const mpcx_retire *retire, const mpcx_scene *scene, int32_t exchange);
int32_t mpcx_admit_prepare(mpcx_ctx *ctx, size_t n_rows);
int32_t mpcx_admit_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *obs_off,
                           const int32_t *obs_cnt, const int32_t *obs_skip, int32_t *done, int32_t n_obs_pool, int32_t *absent,
                           int32_t n_actors, const mpcx_traffic_actor *actors, const double *actor_state, const double *tape,
                           int64_t tape_rows, const int32_t *actor_row, const mpcx_admit *admit);
// respawn (mpcx_respawn.hip): "no respawn" test, check of the struct against the run, the launch alone
bool mpcx_respawn_absent(const mpcx_respawn *s);
int32_t mpcx_respawn_validate(mpcx_ctx *ctx, const mpcx_respawn *s, const mpcx_admit *admit);
int32_t mpcx_respawn_enqueue(mpcx_ctx *ctx, int32_t P, double *state, double *applied, double *u_sol, int32_t *traj_idx, int32_t *target_ind,
                             int32_t *cut_len, int32_t *iters, int32_t *prev_len /*or nullptr*/, const int32_t *obs_skip, int32_t n_obs_pool,
                             const mpcx_run_log *log /*or nullptr*/, const mpcx_retire *retire, const mpcx_admit *admit,
                             const mpcx_respawn *respawn);
// routes (mpcx_route.hip): "no routes" test, check of the struct against the run (reads the R-word tables back), the launch alone -- which
// takes the place of mpcx_respawn_enqueue
bool mpcx_routes_absent(const mpcx_routes *s);
int32_t mpcx_routes_validate(mpcx_ctx *ctx, const mpcx_routes *s, const mpcx_respawn *respawn, const int32_t *path_off, const int32_t *path_len,
                             int32_t max_len /*0: no upper bound*/);
int32_t mpcx_route_enqueue(mpcx_ctx *ctx, int32_t P, double *state, double *applied, double *u_sol, int32_t *traj_idx, int32_t *target_ind,
                           int32_t *cut_len, int32_t *iters, int32_t *prev_len /*or nullptr*/, const int32_t *obs_skip, int32_t n_obs_pool,
                           const mpcx_run_log *log /*or nullptr*/, const mpcx_retire *retire, const mpcx_admit *admit,
                           const mpcx_respawn *respawn, const mpcx_routes *routes);
// right of way (mpcx_precedence.hip): "no precedence" test, check of the struct against the run, the entry-order stamp's launch alone
bool mpcx_precedence_absent(const mpcx_precedence *s);
int32_t mpcx_precedence_validate(mpcx_ctx *ctx, const mpcx_precedence *s, const mpcx_scene *scene, const mpcx_admit *admit);
int32_t mpcx_precedence_enqueue(mpcx_ctx *ctx, int32_t P, const int32_t *obs_off, const int32_t *obs_skip, const mpcx_admit *admit,
                                const mpcx_precedence *precedence);
// traffic signals (mpcx_signal.hip): "no signals" test, check of the struct against the run (reads the plan tables back), the launch alone
bool mpcx_signals_absent(const mpcx_signals *s);
int32_t mpcx_signals_validate(mpcx_ctx *ctx, const mpcx_signals *s, int32_t exchange);
int32_t mpcx_signal_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                            const int32_t *traj_idx, int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_signals *signals);
// vehicle-actuated signals (mpcx_actuated.hip): "no actuation" test, check of both structs against the run (reads the controller tables back),
// the launch alone (in the place of mpcx_signal_enqueue)
bool mpcx_actuation_absent(const mpcx_actuation *s);
int32_t mpcx_actuation_validate(mpcx_ctx *ctx, const mpcx_actuation *s, const mpcx_signals *sg, int32_t P, int32_t exchange);
int32_t mpcx_actuated_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                              const int32_t *traj_idx, int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_signals *signals,
                              const mpcx_actuation *actuation);
// signal-aware approach speed (mpcx_advise.hip): "no advice" test, check of the struct against the run (the signals it draws on are
// checked by mpcx_signals_validate), the launch alone (between the window stage and the QP)
bool mpcx_advice_absent(const mpcx_advice *s);
int32_t mpcx_advise_validate(mpcx_ctx *ctx, const mpcx_advice *s, const mpcx_signals *sg, bool actuated, bool speed, int32_t P);
int32_t mpcx_advise_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx,
                            const int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_signals *signals, const mpcx_advice *advice,
                            double *xref);
// shared plans (mpcx_intent.hip): "no sharing" test, check of the struct against the run (reads obs_skip back), the launch alone (between
// the prediction and the conflict search, inside mpcx_interaction_enqueue)
bool mpcx_intent_absent(const mpcx_intent *s);
int32_t mpcx_intent_validate(mpcx_ctx *ctx, const mpcx_intent *s, int32_t P, int32_t exchange, int32_t pool_rows, const int32_t *obs_skip);
int32_t mpcx_intent_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *obs_skip,
                            int32_t n_obs_pool, const mpcx_intent_launch &x);
// crossing reservations (mpcx_reserve.hip): "no reservations" test, check of both structs against the run (reads conflict, lane and mgr_time
// back), the launch alone (in the place of mpcx_signal_enqueue / mpcx_actuated_enqueue)
bool mpcx_reservation_absent(const mpcx_reservation *s);
int32_t mpcx_reservation_validate(mpcx_ctx *ctx, const mpcx_reservation *s, const mpcx_signals *sg, int32_t P, int32_t exchange, bool actuated,
                                  bool advised);
int32_t mpcx_reserve_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                             const int32_t *traj_idx, int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_signals *signals,
                             const mpcx_reservation *reservation);
// car following (mpcx_follow.hip): "no following" test, check of the struct against the run, the two launches alone (the search behind the
// signal stage or the conflict search, the clamp behind a window stage in speed mode)
bool mpcx_following_absent(const mpcx_following *s);
int32_t mpcx_following_validate(mpcx_ctx *ctx, const mpcx_following *s, int32_t P, int32_t exchange);
int32_t mpcx_follow_enqueue(mpcx_ctx *ctx, int32_t P, double dl, bool speed, const double *state, const double *path_xyyaw,
                            const int32_t *path_off, const int32_t *path_len, const int32_t *traj_idx, int32_t *cut_len,
                            const int32_t *done /*or nullptr*/, int32_t n_obs_pool, const double *obs6, const int32_t *obs_off,
                            const int32_t *obs_cnt, const int32_t *obs_skip /*or nullptr*/, const int32_t *absent /*or nullptr*/,
                            const mpcx_following *following);
int32_t mpcx_follow_cap_enqueue(mpcx_ctx *ctx, int32_t P, const int32_t *done /*or nullptr*/, const mpcx_following *following, double *xref);
// the near-miss log (mpcx_safety.hip): "no safety stage" test, check of the struct against the run (n_pool: its pool rows), the launch alone
// (directly behind the conflict search; pred: n_obs_pool x pred_steps x 4 doubles)
bool mpcx_safety_absent(const mpcx_safety *s);
int32_t mpcx_safety_validate(mpcx_ctx *ctx, const mpcx_safety *s, const mpcx_interaction_params *ip, int32_t P, int32_t n_pool, int32_t exchange);
int32_t mpcx_safety_enqueue(mpcx_ctx *ctx, const mpcx_interaction_params *ip, int32_t P, const double *state, const int32_t *path_off,
                            const int32_t *traj_idx, const int32_t *done /*or nullptr*/, int32_t n_obs_pool, const double *obs6,
                            const double *pred, const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip,
                            const int32_t *absent /*or nullptr*/, const mpcx_safety *safety);
// line of sight (mpcx_sight.hip): "no sight stage" test, check of the struct against the run (n_pool: its pool rows; reads the two offset
// tables back), the launch alone (in front of the conflict search, on the pool as packed)
bool mpcx_sight_absent(const mpcx_sight *s);
int32_t mpcx_sight_validate(mpcx_ctx *ctx, const mpcx_sight *s, int32_t P, int32_t n_pool);
int32_t mpcx_sight_enqueue(mpcx_ctx *ctx, int32_t P, const double *state, const int32_t *done /*or nullptr*/, int32_t n_obs_pool,
                           const double *obs6, const int32_t *obs_off, const int32_t *obs_cnt, const int32_t *obs_skip,
                           const int32_t *absent /*or nullptr*/, const mpcx_sight *sight);
// keep clear (mpcx_keepclear.hip): "no keep-clear stage" test, check of the struct against the run (sg: the run's signals or nullptr;
// reserved_run: the run also carries a reservation; reads the conflict table back once per struct), the launch alone (behind the hold, in
// front of the following stage)
bool mpcx_keepclear_absent(const mpcx_keepclear *s);
int32_t mpcx_keepclear_validate(mpcx_ctx *ctx, const mpcx_keepclear *s, const mpcx_signals *sg, int32_t P, int32_t exchange, bool reserved_run);
int32_t mpcx_keepclear_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                               const int32_t *traj_idx, int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_signals *signals,
                               const mpcx_keepclear *keepclear);
// priority road (mpcx_priority.hip): "no priority stage" test, check of the struct against the run (held_run: the run carries signals,
// actuation or a reservation; reads the three per-movement tables back once per struct), the launch alone (in the hold's place)
bool mpcx_priority_absent(const mpcx_priority *s);
int32_t mpcx_priority_validate(mpcx_ctx *ctx, const mpcx_priority *s, int32_t P, int32_t exchange, bool held_run);
int32_t mpcx_priority_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                              const int32_t *traj_idx, int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_priority *priority);
// stop signs (mpcx_stopsign.hip): "no stop-sign stage" test, check of the struct against the run (other: what else runs the junction in
// this run, nullptr = nothing), and the launch alone
bool mpcx_stopsign_absent(const mpcx_stopsign *s);
int32_t mpcx_stopsign_validate(mpcx_ctx *ctx, const mpcx_stopsign *s, int32_t P, int32_t exchange, const char *other);
int32_t mpcx_stopsign_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const int32_t *path_off, const int32_t *path_len,
                              const int32_t *traj_idx, int32_t *cut_len, const int32_t *done /*or nullptr*/, const mpcx_stopsign *stopsign);
// firm hold (mpcx_brake.hip): "no firm hold" test, check of the struct against the run (lines: the run has a source of stop lines), the two
// launches alone (the mark in front of the window stage, the clamp behind it in speed mode)
bool mpcx_braking_absent(const mpcx_braking *s);
int32_t mpcx_braking_validate(mpcx_ctx *ctx, const mpcx_braking *s, double dl, int32_t exchange, int32_t lin_passes, bool lines);
int32_t mpcx_brake_mark_enqueue(mpcx_ctx *ctx, int32_t P, double dl, bool speed, const int32_t *path_off, const int32_t *path_len,
                                const int32_t *traj_idx, int32_t *target_ind, int32_t *win_len, const int32_t *done /*or nullptr*/,
                                const int32_t *path_stop, int32_t n_points, const int32_t *held, const int32_t *boxed, const int32_t *yielding,
                                const mpcx_braking *braking);
int32_t mpcx_brake_clamp_enqueue(mpcx_ctx *ctx, int32_t P, double dl, const double *state, const double *path_xyyaw, const int32_t *path_off,
                                 const int32_t *path_len, int32_t *traj_idx, int32_t *len_seen /*or nullptr*/, const int32_t *done /*or nullptr*/,
                                 const int32_t *path_stop, int32_t n_points, const mpcx_braking *braking, double *xref);
int32_t mpcx_ensure_ticket(mpcx_ctx *ctx);                    // work-queue word (mpcx_qp.hip)
// Work-queue key: expected length of a solve.  hint = the previous step's iteration count; a problem whose path cut moved since
// the previous step starts far from its warm start and is counted as MPCX_JUMP_BONUS iterations (mpcx_qp.hip has the measurements).
#define MPCX_JUMP_BONUS 11
#define MPCX_ORDER_BINS 64
#define MPCX_TICKET_WORDS 8      /* ctx->ticket: the queue head and the other per-launch counters, zeroed together */
#define MPCX_TICKET_QUEUE_LEN 6  /* ... of which this word holds the length of the step's queue under retirement (written by the window stage) */
#define MPCX_ORDER_COPIES 16
namespace mpcx {
__device__ __forceinline__ int order_key_of(int hint, bool moved) {
    int k = hint < 0 ? 0 : hint;
    if (moved) k += MPCX_JUMP_BONUS;
    return k < MPCX_ORDER_BINS ? k : MPCX_ORDER_BINS - 1;
}
}
int32_t mpcx_ensure_order(mpcx_ctx *ctx, size_t B);             // work-queue order scratch (mpcx_qp.hip)
// counting sort of the work queue on stream st from (hint, now, prev) into ctx->order; also zeroes the ticket (mpcx_qp.hip)
int32_t mpcx_qp_build_order(mpcx_ctx *ctx, int32_t B, const int32_t *hint, const int32_t *now, const int32_t *prev, hipStream_t st);

namespace mpcx {

constexpr int WAVE = 64;

struct QpArgs {
    mpcx_mpc_params p;
    int B;
    int32_t *ticket;      // work queue head (zeroed before the launch): wavefronts draw QP indices until B is exhausted
    int has_warm;         // u_warm != NULL (tested on the host: a device-side null test of a kernel-argument pointer trips a
                          // gfx950 instruction-selection bug in some register-allocation outcomes)
    const double *x0, *xref, *xbar, *u_warm;
    const uint8_t *re;
    double *x_out, *u_out, *kkt;
    int32_t *status, *iters;
    const mpcx_qp_tuning *tune;   // per-problem rows or nullptr
    int has_tune;                 // tune != NULL, tested on the host like has_warm
    const int32_t *order;         // ticket -> problem index (hard problems first) or nullptr = identity
    int has_order;
    // second chance for problems the condensed solver gives up on (MAXITER / NUMERIC): with defer_fail it leaves their outputs
    // untouched and appends their indices to fail_list; the stage solver then runs over that list, whose length it reads from
    // *queue_len (has_queue_len) instead of B.  The closed loop with retirement at the goal passes the first launch a queue_len of its own:
    // the number of agents filed in this step's queue (both solvers draw tickets up to it)
    int defer_fail;
    int32_t *fail_list, *fail_count;
    const int32_t *queue_len;
    int has_queue_len;
    int plain_rounds;             // stage solver: rounds without a trial or polishing problem run the plain copies of the row passes (mpcx_qp_set_plain_rounds)
};

void launch_qp_stage(const QpArgs &a, hipStream_t st, int n_cu);   // mpcx_qp_quad.hip
int qp_stage_grid(int B, int n_cu);                                 // wavefronts launch_qp_stage starts for B problems (mpcx_qp_quad.hip)

__device__ __forceinline__ double rdlane(double v, int l) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}
// 1/d: hardware seed + two Newton steps (full double accuracy, not correctly rounded)
__device__ __forceinline__ double frcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}

// ---------------------------------------------------------------- DPP cross-lane helpers (no LDS round trip)
// gfx9 DPP controls: row_shl:n 0x100+n, row_shr:n 0x110+n, wave_shl:1 0x130, wave_shr:1 0x138, row_bcast:15 0x142,
// row_bcast:31 0x143.  A "row" is 16 consecutive lanes.  Lanes whose source is out of range keep `old`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_mov(double old, double src) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, ROW_MASK, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
// value of lane+1 / lane-1 (wave-wide shift by one; the edge lane gets `fill`)
__device__ __forceinline__ double lane_next(double v, double fill = 0.0) { return dpp_mov<0x130>(fill, v); }
__device__ __forceinline__ double lane_prev(double v, double fill = 0.0) { return dpp_mov<0x138>(fill, v); }

// inclusive prefix sum over lanes 0..31 (rows 0 and 1); lanes >= 32 return garbage-free but meaningless values
__device__ __forceinline__ double scan_up32(double v) {
    v += dpp_mov<0x111>(0.0, v);
    v += dpp_mov<0x112>(0.0, v);
    v += dpp_mov<0x114>(0.0, v);
    v += dpp_mov<0x118>(0.0, v);
    v += dpp_mov<0x142, 0xA>(0.0, v);      // row_bcast:15 into rows 1 and 3: add the previous row's total
    return v;
}
// inclusive suffix sum over lanes 0..31: lane i gets sum of lanes i..31
__device__ __forceinline__ double scan_down32(double v, int lane) {
    v += dpp_mov<0x101>(0.0, v);
    v += dpp_mov<0x102>(0.0, v);
    v += dpp_mov<0x104>(0.0, v);
    v += dpp_mov<0x108>(0.0, v);
    const double r1 = rdlane(v, 16);       // total of row 1
    return v + ((lane < 16) ? r1 : 0.0);
}
// wave-wide reductions whose result is wave-uniform (lanes 0..63)
__device__ __forceinline__ double wave_sum_dpp(double v) {
    v += dpp_mov<0x111>(0.0, v);
    v += dpp_mov<0x112>(0.0, v);
    v += dpp_mov<0x114>(0.0, v);
    v += dpp_mov<0x118>(0.0, v);           // lane 15 of each row holds the row total
    return (rdlane(v, 15) + rdlane(v, 31)) + (rdlane(v, 47) + rdlane(v, 63));
}
__device__ __forceinline__ double wave_max_dpp(double v) {
    v = fmax(v, dpp_mov<0x111>(v, v));
    v = fmax(v, dpp_mov<0x112>(v, v));
    v = fmax(v, dpp_mov<0x114>(v, v));
    v = fmax(v, dpp_mov<0x118>(v, v));
    return fmax(fmax(rdlane(v, 15), rdlane(v, 31)), fmax(rdlane(v, 47), rdlane(v, 63)));
}
// 1/d with ONE Newton step on the hardware seed (~1e-15 relative; used where the consumer is itself iterative)
__device__ __forceinline__ double frcp1(double d) {
    double r = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, r, 1.0), r, r);
}

// lexicographic (distance, index) minimum over the wave
__device__ __forceinline__ void wave_argmin(double &d, int &i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        double od = __shfl_xor(d, s, WAVE);
        int oi = __shfl_xor(i, s, WAVE);
        bool take = (od < d) || (od == d && oi < i);
        d = take ? od : d;
        i = take ? oi : i;
    }
}

template <typename T>      // int, long long
__device__ __forceinline__ T wave_min_i(T v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { T o = __shfl_xor(v, s, WAVE); v = o < v ? o : v; }
    return v;
}

// A recurrence acc_i = f(acc_{i-1}, term_i) over the G consecutive lanes of a group (G a power of two, lane j of the group holds term_j),
// evaluated strictly in index order: every lane runs the whole chain on shuffled terms -- the same operations on the same operands as one
// lane walking it alone, so the same bits -- and keeps the value of its own index.  Returns acc_j; leaves acc = acc_{G-1} in every lane,
// the carry into the group's next G indices.  What is expensive per index (sincos, tan, divide) goes into the terms, one index per lane;
// only f, an addition or so, is serial.  SAME: the term is the same in every lane (no shuffle).
template <int G, bool SAME = false, class F>
__device__ __forceinline__ double group_chain(double &acc, double term, int j, F f) {
    double mine = acc;
#pragma unroll
    for (int i = 0; i < G; i++) {
        acc = f(acc, SAME ? term : __shfl(term, i, G));
        mine = i == j ? acc : mine;
    }
    return mine;
}
// the value the previous index left: lane j - 1's, or `first` in lane 0 of the group
template <int G>
__device__ __forceinline__ double group_prev(double v, double first, int j) {
    const double up = __shfl_up(v, 1, G);
    return j == 0 ? first : up;
}

// trajectories.py:11-37: centre (ex, ey) of the disc at (cx, cy) in the frame of a pose at (px, py) whose heading has cos / sin (c, s)
__device__ __forceinline__ void disc_centre(double px, double py, double c, double s, double cx, double cy, double &ex, double &ey) {
    ex = __dadd_rn(__dadd_rn(__dmul_rn(c, cx), -__dmul_rn(s, cy)), px);
    ey = __dadd_rn(__dadd_rn(__dmul_rn(s, cx), __dmul_rn(c, cy)), py);
}

// One lane's three smallest (distance, index) pairs of the points offered to it, ascending, ties by lower index (= numpy's argpartition +
// argsort on these data), with their squared distances.  The conflict search (interaction_kernel) and the window selection
// (nearest_index_in_direction) both take their three nearest path points from here: the window kernel uses the conflict search's answer as
// its own (mpcx_interaction_extras::near), so the two must agree bit for bit.
struct Top3 {
    double d0 = INFINITY, d1 = INFINITY, d2 = INFINITY, s2 = INFINITY, s1 = INFINITY, s0 = INFINITY;
    int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;
    // point i at (px, py), ego at (x, y).  The square root is taken only where the squared distance could enter the lane's three (sqrt is
    // monotone, so a larger square cannot give a smaller distance).
    __device__ __forceinline__ void offer(double px, double py, double x, double y, int i) {
        const double dx = __dadd_rn(px, -x), dy = __dadd_rn(py, -y);
        const double q = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (q < s2 || i2 == 0x7fffffff) {
            const double d = __dsqrt_rn(q);
            if (d < d2 || (d == d2 && i < i2)) {
                if (d < d1 || (d == d1 && i < i1)) {
                    d2 = d1; i2 = i1; s2 = s1;
                    if (d < d0 || (d == d0 && i < i0)) { d1 = d0; i1 = i0; s1 = s0; d0 = d; i0 = i; s0 = q; }
                    else { d1 = d; i1 = i; s1 = q; }
                } else { d2 = d; i2 = i; s2 = q; }
            }
        }
    }
    // the indices of the wave's three smallest pairs, ascending: pop the wave-wide minimum three times (consumes the lanes' entries)
    __device__ __forceinline__ void pop3(int (&bi)[3]) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double d = d0; int ix = i0;
            wave_argmin(d, ix);
            bi[r] = ix;
            if (i0 == ix) { d0 = d1; i0 = i1; d1 = d2; i1 = i2; d2 = INFINITY; i2 = 0x7fffffff; }
        }
    }
};
// trajectories.py:117-126 on the three nearest indices (ascending distance): the nearest if its neighbours straddle it, else the forward one
// of two adjacent nearest, else -1 ("something wrong")
__device__ __forceinline__ int three_nearest(const int (&bi)[3], int base) {
    if (abs(bi[1] - bi[2]) == 2) return bi[0] + base;
    if (abs(bi[0] - bi[1]) == 1) return max(bi[0], bi[1]) + base;
    return -1;
}

// trajectories.py:100-126 on path[start .. n) ; returns absolute index or -1 ("something wrong").  ONE pass over the points keeps each lane's
// three smallest (Top3; the next 64 points are in flight meanwhile).  Round 1 made three passes with a square root per point each.
__device__ inline int nearest_index_in_direction(const double *path, int n, int start, double x, double y, int lane) {
    const int len = n - start;
    if (len <= 1) return start;
    if (len == 2) return start + 1;
    Top3 top;
    // the points arrive in batches of DEPTH x 64 with the next batch's loads all in flight (one batch deep the scan waited for an
    // L2 round trip per 64 points: there is almost no arithmetic to hide it behind)
    constexpr int DEPTH = 4;
    double bx[DEPTH], by[DEPTH];
#pragma unroll
    for (int k = 0; k < DEPTH; k++) {
        const int i = k * WAVE + lane;
        const double *q = path + 3 * (size_t)(start + (i < len ? i : 0));        // clamped address, selected afterwards
        const double vx = q[0], vy = q[1];
        bx[k] = vx; by[k] = vy;
    }
    for (int i0 = 0; i0 < len; i0 += DEPTH * WAVE) {
        double nbx[DEPTH], nby[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            const int i = i0 + (DEPTH + k) * WAVE + lane;
            const double *q = path + 3 * (size_t)(start + (i < len ? i : 0));
            nbx[k] = q[0]; nby[k] = q[1];
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            const int i = i0 + k * WAVE + lane;
            if (i < len) top.offer(bx[k], by[k], x, y, i);
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) { bx[k] = nbx[k]; by[k] = nby[k]; }
    }
    int bi[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {     // Top3::pop3 written out: through the member ref_window_kernel measured 33.59 us against 33.41 (other register allocation)
        double d = top.d0; int ix = top.i0;
        wave_argmin(d, ix);
        bi[r] = ix;
        if (top.i0 == ix) { top.d0 = top.d1; top.i0 = top.i1; top.d1 = top.d2; top.i1 = top.i2; top.d2 = INFINITY; top.i2 = 0x7fffffff; }
    }
    return three_nearest(bi, start);
}

}  // namespace mpcx
