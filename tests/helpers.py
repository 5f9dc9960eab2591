"""Shared test helpers: golden fixtures (tests/golden, generated from the reference by make_golden.py) and
model builders. Nothing here reads /root/reference."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_cache = {}


def gold(name):
    if name not in _cache:
        path = os.path.join(GOLD, name)
        if name.endswith('.json'):
            with open(path) as f:
                _cache[name] = json.load(f)
        else:
            _cache[name] = np.load(path)
    return _cache[name]


def prim_meta(version='bicycle_model'):
    return gold('primitives_meta.json')[version]


def car(version='bicycle_model'):
    return gold('primitives_meta.json')['cars'][version]


def search_tables(version='bicycle_model', scenario='int_4_1'):
    """(templates, last_pose, edge_cost, hp, hp_off) with primitive ids = sorted names"""
    meta = prim_meta(version)
    prim, tm, sc = gold('primitives.npz'), gold('templates.npz'), gold('scenarios.npz')
    names = meta['names']
    templates = [tm['%s/%s' % (version, n)] for n in names]
    last = np.array([prim['%s/%s' % (version, n)][-1] for n in names])
    tag = 'bic' if version == 'bicycle_model' else 'pri'
    return templates, last, np.array(meta['total_length']), sc[scenario + '/hp_' + tag], sc[scenario + '/hp_off']


def smoothed_path(sp, ti):
    """A* trajectory of intersection(sp, ti) with the yaw column unwrapped as MPC.__init__ does (mpc.py:257)."""
    from oracle import oracle_py as orc
    full = gold('mpc_pre.npz')['path_%d_%d' % (sp, ti)].copy()
    full[:, 2] = orc.smooth_yaw(full[:, 2])
    return full


def ego_resample_dl(n, v0, dt=0.2, max_accel=2.0, max_speed=30.0 / 3.6):
    """scenarios/mpc_intersection.py:110-116 (caller code): the dl passed to resample_curve"""
    if v0 < max_speed:
        return dt * np.minimum(np.cumsum(np.zeros(n) + max_accel) + v0, max_speed)
    return dt * max_speed


def harvest_closed_loop_qps(ctx, B=4096, A=8, T=20, seed=1000, windows=((3, 6), (100, 6)), hard_iters=10, total=4096, rng_seed=0, mpc=None):
    """QP inputs out of the benchmark's closed loop (bench.py's workload: synthetic_batch(seed=1000)): for every step of the
    windows [(first step, how many), ...] EVERY problem that took >= hard_iters interior-point iterations, topped up with a random
    sample of the other problems of those steps to `total`.  Inputs are taken as the QP kernel saw them: x0 = column 0 of its state
    output, reference window / linearisation points of the step, warm start = the previous solution.
    Returns dict of numpy arrays: x0, xref, xbar, re, uw, iters (of the closed-loop solve), step."""
    import torch
    from mpc_for_av_at_intersection_amd.batch import synthetic_batch
    sim = synthetic_batch(ctx, B=B, A=A, T=T, seed=seed, mpc=mpc)       # mpc: other controller constants (e.g. MpcParams.jerk()); its T wins
    rng = np.random.default_rng(rng_seed)
    hard, rest = [], []
    n_steps = sum(n for _, n in windows)
    quota = max(0, total // max(1, n_steps))
    for first, n in windows:
        if first > sim.steps_done:
            sim.run(first - sim.steps_done)
        for _ in range(n):
            uw = sim.sol['u'].clone()
            sim.step()
            it = sim.sol['iters']
            hi = torch.nonzero(it >= hard_iters).flatten()
            lo = torch.nonzero(it < hard_iters).flatten()
            lo = lo[torch.as_tensor(rng.choice(len(lo), min(quota, len(lo)), replace=False), device=lo.device)]
            for idx, dst in ((hi, hard), (lo, rest)):
                dst.append(dict(x0=sim.sol['x'][idx][:, :, 0].cpu().numpy(), xref=sim.pre['xref'][idx].cpu().numpy(),
                                xbar=sim.pre['xbar'][idx].cpu().numpy(), re=sim.pre['reaches_end'][idx].cpu().numpy(),
                                uw=uw[idx].cpu().numpy(), iters=it[idx].cpu().numpy(),
                                step=np.full(len(idx), sim.steps_done, dtype=np.int32)))
    cat = lambda rows, k: np.concatenate([r[k] for r in rows])
    out = {k: cat(hard, k) for k in hard[0]}
    n_rest = max(0, total - len(out['iters']))
    r = {k: cat(rest, k) for k in rest[0]}
    keep = rng.choice(len(r['iters']), min(n_rest, len(r['iters'])), replace=False)
    return {k: np.concatenate([out[k], r[k][keep]]) for k in out}


HORIZON_FIXTURE_TS = (1, 2, 9, 11, 14, 16, 17, 21, 24, 25, 30, 31, 32)     # mpc_pre_horizons.npz (make_golden.py --stage horizons)


def pre_gold(T):
    """the T%d/* window / rollout block for horizon T: mpc_pre.npz holds T = 10 / 13 / 20, mpc_pre_horizons.npz the others"""
    return gold('mpc_pre.npz') if T in (10, 13, 20) else gold('mpc_pre_horizons.npz')


def _fit(a, T):
    """a control sequence cut or extended (last value held) to T entries"""
    return a[:T] if len(a) >= T else np.concatenate([a, np.full(T - len(a), a[-1])])


def horizon_problems(T, n=12, every=1):
    """QP inputs at horizon T built by the oracle from golden cases (those of T itself where a fixture has them, else those of the
    nearest fixture horizon): states, cut paths and starts of the fixture, reference window and rollout made at T.  Each case gives two
    problems, as two steps of a closed loop: (1) the rollout of the fixture's random controls, those controls as warm start; (2) the state
    the plant reaches under (1)'s solution, its window from (1)'s target index, its rollout made with (1)'s solution and that solution as
    warm start.  Returns a list of (x0, xref, xbar, re, u_warm)."""
    from oracle import oracle_py as orc
    have = (10, 13, 20) + HORIZON_FIXTURE_TS
    src = min(have, key=lambda t: (abs(t - T), t))
    g = pre_gold(src)
    p = orc.MpcParams(T=T)
    out = []
    for k in range(0, min(n * every, len(g['T%d/state' % src])), every):
        sp, ti, cut = g['T%d/path' % src][k]
        full = smoothed_path(sp, ti)
        path = full[:cut]
        dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
        st = g['T%d/state' % src][k]
        xref, s, re = orc.calc_ref_trajectory(p, st, path[:, 0], path[:, 1], path[:, 2], dl, int(g['T%d/start' % src][k]))
        if s < 0:
            continue
        uw = np.stack([_fit(g['T%d/oa' % src][k], T), _fit(g['T%d/od' % src][k], T)])
        xbar = orc.predict_motion(p, st, uw[0], uw[1])
        out.append((st, xref, xbar, re, uw))
        sol = orc.qp_solve(p, st, xref, xbar, re, uw)
        if sol.status != 0:
            continue
        st2 = orc.plant_step(p, st, sol.u[0, 0], sol.u[1, 0])
        xref2, s2, re2 = orc.calc_ref_trajectory(p, st2, path[:, 0], path[:, 1], path[:, 2], dl, s)
        if s2 < 0:
            continue
        out.append((st2, xref2, orc.predict_motion(p, st2, sol.u[0], sol.u[1]), re2, sol.u.copy()))
    return out


def stack_problems(probs):
    """list of (x0, xref, xbar, re, u_warm) -> five stacked arrays (re as uint8)"""
    return [np.stack([q[i] for q in probs]).astype(np.uint8 if i == 3 else np.float64) for i in range(5)]


def replay_all_on_oracle(sim, before, after, threads=16, tol=2e-7, dead=None):
    """EVERY agent of the step before -> after replayed on the oracle (orc_agent_steps_mt: the whole per-agent step in C, pthreads
    over agents) from the device state `before`: integer decisions and solver status must be identical for every agent, solutions
    within tol -- ONE tolerance for every agent, whatever its iteration count: since the active-set polish of round 3 both sides end
    on the same KKT point even where an exit test on the edge of its tolerance sends them there by different routes.  Returns (worst
    |solution difference|, agents whose iteration count differs, failed solves)."""
    from oracle import oracle_py as orc
    import dataclasses
    po = orc.MpcParams(**{f.name: getattr(sim.params, f.name) for f in dataclasses.fields(orc.MpcParams)})
    tab = sim.path.cpu().numpy(); off = sim.path_off.cpu().numpy(); ln = sim.path_len.cpu().numpy()
    r = orc.agent_steps_batch(po, threads, sim.A, tab, off, ln, sim.dl, before['state'], before['applied'], before['u'],
                              before['traj_idx'], before['prev_cut'], before['target_ind'],
                              np.asarray(sim.ip.circle_centers).reshape(2, 2), sim.ip.radius, sim.ip.cutoff_margin,
                              pred_steps=sim.ip.pred_steps, frame_window=sim.ip.frame_window, max_accel=sim.ip.max_accel)
    o = r['out6']
    # where the reference raises Exception('something wrong') (trajectories.py:120: the three nearest path points are not
    # contiguous) the oracle stops (index -1) and the kernels flag the agent: hit_idx -3 (conflict search) / target_ind -1
    # (agents in `dead` raised on an earlier step: the reference's run ended there, they are not followed any further)
    dead = np.zeros(len(o), bool) if dead is None else dead
    raised_a, raised_b = (o[:, 0] < 0) & ~dead, (o[:, 0] >= 0) & (o[:, 2] < 0) & ~dead
    assert np.array_equal((after['hit_idx'] == -3) & ~dead, raised_a) and np.array_equal((after['target_ind'] < 0) & ~raised_a & ~dead, raised_b)
    live = ~(raised_a | raised_b | dead)
    sim.raised = raised_a | raised_b
    for col, name in ((0, 'traj_idx'), (1, 'cut_len'), (2, 'target_ind'), (3, 'hit_idx'), (4, 'status')):
        bad = np.nonzero((o[:, col] != after[name]) & live)[0]
        assert len(bad) == 0, '%s differs from the oracle for %d agents, first %s: %s vs %s' % (name, len(bad), bad[:5], after[name][bad[:5]], o[bad[:5], col])
    ok = (after['status'] == 0) & live
    diff = np.maximum(np.abs(r['u'] - after['u']).max((1, 2)), np.abs(r['x'] - after['x']).max((1, 2)))
    same_count = o[:, 5] == after['iters']
    worst = float(diff[ok].max()) if ok.any() else 0.0
    assert worst < tol, (worst, int(diff[ok].argmax()))
    return worst, int((~same_count).sum()), int((~ok).sum())


WIDE_CHUNK = 512        # obstacle disc positions the conflict-search kernel holds per pass of its candidate loop (8 per lane)
WIDE_KINDS = {1: 'a', 2: 'b', 3: 'c', 4: 'd', 5: 'e', 6: 'f'}      # moving_wide.npz: `kind` of the constructed cases (0 = random)


def wide_cases():
    """moving_wide.npz (make_golden.py --stage moving_wide) as a dict of arrays: idx, v0, nobs, steps, window split out of `in`, + the rest"""
    g = gold('moving_wide.npz')
    out = {k: g[k] for k in g.files}
    cols = out.pop('in')
    out['v0'] = cols[:, 1]
    for j, k in ((0, 'idx'), (2, 'nobs'), (3, 'steps'), (4, 'window')):
        out[k] = cols[:, j].astype(np.int32)
    return out


def wide_coverage(w):
    """The conditions make_golden.py asserted when it recorded moving_wide.npz, from the stored arrays alone (a regenerated fixture cannot
    lose them quietly).  Returns (hits at steps >= 35, those whose winner's candidates start in a later chunk) of the random part."""
    rnd, hit = w['kind'] == 0, w['hit'][:, 2] >= 0
    cells = sorted(set(zip(w['steps'][rnd].tolist(), w['window'][rnd].tolist())))
    assert cells == [(s, f) for s in (1, 2, 7, 35, 36, 50, 63, 64) for f in (0, 3, 20, 40, 70)]
    for s, f in cells:
        cell = rnd & (w['steps'] == s) & (w['window'] == f)
        assert cell.sum() == 20 and (hit & cell).sum() >= 3 and (~hit & cell).sum() >= 2, (s, f)
    assert w['nobs'][rnd].min() == 8 and w['nobs'][rnd].max() == 16 and (w['nobs'][~rnd] == 16).all()
    assert ((w['winner_rank'] >= 0) == hit).all() and (w['winner_rank'] < w['nobs']).all()
    long_hits = rnd & hit & (w['steps'] >= 35)
    late = long_hits & (w['winner_rank'] * w['steps'] * 2 >= WIDE_CHUNK)
    assert 4 * late.sum() >= long_hits.sum(), (int(late.sum()), int(long_hits.sum()))
    for rel in (np.less, np.equal, np.greater):
        assert rel(w['nres'][rnd], w['steps'][rnd]).any()
    k, r, win = w['kind'], w['rank'], w['winner_rank']
    for steps in (35, 64):
        at = w['steps'] == steps
        for kind in (1, 5):                                     # (a), (e): the winner is the one near obstacle, at every rank
            assert sorted(r[at & (k == kind)].tolist()) == list(range(16)) and (win[at & (k == kind)] == r[at & (k == kind)]).all()
        assert win[at & (k == 2)].tolist() == [15] and win[at & (k == 3)].tolist() == [0]            # (b), (c)
        assert win[at & (k == 4)].tolist() == [2, 13]           # (d): both near obstacles, then rank 13 alone
        assert (w['nres'][at & (k == 5)] < steps).all()         # (e): the ego's prediction is the shorter one
    f = k == 6
    assert (w['steps'][f] == 2).all() and sorted(r[f].tolist()) == list(range(16)) and (win[f] == r[f]).all() and (w['nres'][f] > 30).all()
    return int(long_hits.sum()), int(late.sum())
