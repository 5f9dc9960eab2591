// mpcx_interaction_kernel_body.h -- NOT a header in its own right: the statements of the conflict search's kernel, included inside the body
// of interaction_kernel<RETIRE, SCENE, PREC>(InterArgs a) and of interaction_sight_kernel<PREC>(InterSightArgs a) in
// mpcx_interaction_parts.h, which define RETIRE, SCENE and PREC (template parameters or constants) and MPCX_INTERACTION_SIGHT (0 or 1) around
// the #include.  Kept as text, not as a function the kernels call: interaction_kernel then compiles to the very bytes it compiled to before
// there was line of sight (a common __device__ body, by reference or by value, changed its register allocation).
    // a retired agent: nothing is read, written or filed -- its outputs stay as its last driven step left them, and an agent that is
    // not filed is never solved (predict_kernel has packed its pool row all the same: to the others it is a parked car)
    if constexpr (RETIRE) { if (a.done[blockIdx.x] != 0) return; }
    // dynamic LDS, sized by the host from the longest path of the call (mpcx_interaction_params.max_path_len):
    //   s_cum [max_rem] doubles   step / cumulative lengths of the remaining path; once the resampling has consumed them the
    //                             same bytes hold s_ego [fcap][4] (ego disc centres per kept pose) and s_box (the runs' boxes)
    //   s_keep [fcap] shorts      indices of the kept poses
    // (round 4: no static LDS, 16-bit indices, no candidate queue: 6464 B at the benchmark's capacity.  Six wavefronts per SIMD -- launch bound 6: 80 VGPRs, 64 B/lane of
    // scratch -- measured 0.138 ms against 0.122 at five: the kernel is bound by instruction issue, more wavefronts only share it)
    extern __shared__ double s_dyn[];
    const int MAXREM = a.max_rem, MAXF = a.fcap;
    double *s_cum = s_dyn;
    unsigned short *s_keep = reinterpret_cast<unsigned short *>(s_dyn + MAXREM);             // (indices < max_rem <= 4096)
    double (*s_ego)[4] = reinterpret_cast<double (*)[4]>(s_cum);
    double (*s_box)[4] = reinterpret_cast<double (*)[4]>(s_cum + (size_t)MAXF * 4);           // bounding boxes of the ego discs per run of frames (256 B behind s_ego)

    const int p = blockIdx.x, lane = threadIdx.x;
    const mpcx_interaction_params &ip = a.ip;
    const size_t poff = (size_t)a.path_off[p];
    const double *path = a.path + 3 * poff;
    const int len = a.path_len[p];
    const double x = a.state[4 * p], y = a.state[4 * p + 1], v = a.state[4 * p + 2];
    const int t_old = a.traj_idx[p];
    const int pcut = a.prev_cut ? a.prev_cut[p] : 0;
    const int kprev = a.key_prev ? a.key_prev[p] : pcut;
    if (a.prev_save && lane == 0) a.prev_save[p] = kprev;
    int nobs;
    RowList rows = {0, 0};
    unsigned yields = 0u;
    if constexpr (SCENE) {
        const int cnt = a.obs_cnt[p];
#if MPCX_INTERACTION_SIGHT      // line of sight: a row the agent cannot see is, for it and only for it, an absent row
        const unsigned long long present = present_rows(a, p, lane, cnt, a.obs_off[p], a.obs_skip ? a.obs_skip[p] : -1) & a.sight[p];
#else
        const unsigned long long present = present_rows(a, p, lane, cnt, a.obs_off[p], a.obs_skip ? a.obs_skip[p] : -1);     // wave-uniform
#endif
        nobs = cnt > WAVE ? MPCX_MAX_OBS + 1 : __popcll(present);       // (beyond one ballot, or too many: locate() leaves with -2)
        if (nobs <= MPCX_MAX_OBS) rows = RowList::of(present);
        if constexpr (PREC) {
            if (nobs <= MPCX_MAX_OBS) yields = yields_by_rank(present, yielding_rows(a, lane, cnt, a.obs_off[p], a.obs_skip ? a.obs_skip[p] : -1, present));
        }
    } else
        nobs = a.obs_cnt[p] - ((a.obs_skip && a.obs_skip[p] >= 0) ? 1 : 0);
    const double *cumtab = ip.path_cum ? ip.path_cum + poff : nullptr;

    const int tidx = locate(a, p, lane, path, len, t_old, x, y, pcut, nobs, cumtab != nullptr, s_cum);
    if (tidx < 0) { leave(a, p, lane, kprev, len, tidx); return; }
    if (lane == 0) a.traj_idx[p] = tidx;
    if (nobs <= 0) { leave(a, p, lane, kprev, len, -1); return; }    // collision_avoidance.py:69-70
    __syncthreads();

    const double dl_const = __dmul_rn(ip.dt, ip.max_speed);
    const Ego e{ip, lane, MAXF, s_cum, s_keep, cumtab,
                path + 3 * (size_t)tidx,              // trajectory = trajectory_full[traj_agent_idx:]
                tidx, tidx - t_old, len - tidx, v, v < ip.max_speed, dl_const, frcp(dl_const),
                cumtab ? cumtab[tidx] : 0.0, cumtab ? ip.path_cum_err + 1e-13 : 1.01e-10};
    const double *rcs = a.path_cs + 2 * (poff + tidx);
    const size_t prow = poff + tidx;
    bool from_plan;
    const int na = ego_frames(e, prow, s_ego, s_box, from_plan);
    if (na > MAXF) { leave(a, p, lane, kprev, len, -2); return; }
    __syncthreads();
    if (!from_plan) ego_discs(e, rcs, na, s_ego);      // else: poses, discs and boxes came from the table
    __syncthreads();
    // conflict search (+ scan of the detailed path on a hit)
    const int ooff = a.obs_off[p], oskip = a.obs_skip ? a.obs_skip[p] : -1;
    double hx, hy;
    const double *pdisc = ip.plan_cnt ? ip.path_disc + 4 * prow : nullptr;     // disc centres of trajectory_full[tidx:] from the host's table
    const int first = first_conflict<SCENE, PREC>(ip, s_ego, na, a.pred, ooff, nobs, oskip, e.rem, rcs, e.n, s_box, lane, hx, hy, from_plan, pdisc, rows,
                                                  a.stand, yields);
    if (first < 0) { leave(a, p, lane, kprev, len, -1); return; }
    finish(a, p, lane, kprev, first, hx, hy, cut_index(ip, path, poff, len, tidx, tidx + first, hx, hy, lane));
