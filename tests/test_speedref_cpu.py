"""CPU tests of the speed-reference stop mode: the reference's recorded run of main/scenarios/mpc_intersection_new_ref.py:90-159 on path
(1, 1) (tests/golden/closedloop_speedref.npz, written by tests/golden/make_golden_speedref.py) replayed step by step on the oracle's
pieces (tests/speedref_helpers.agent_step), and the reference's 999 quirk on a path of more than 1000 points."""
import numpy as np

from tests import helpers as H
from tests import speedref_helpers as S

CTRL_TOL = 1e-9         # oracle vs golden, the bar of test_oracle_golden.test_successive_linearisation_golden


def _car():
    cd = H.car()
    return np.asarray(cd['circle_centers'], float).reshape(2, 2), float(cd['radius'])


def test_golden_run_is_the_run_the_fixture_was_made_for():
    g = H.gold('closedloop_speedref.npz')
    n = int(g['steps'])
    assert n == 88 and len(g['full']) == 720 and len(g['state']) == n
    assert int((g['stop'] != S.NO_STOP).sum()) == 40 and (g['status'] == 0).all()
    assert np.array_equal(g['hit'][:, 2] >= 0, g['stop'] != S.NO_STOP)
    assert float(g['v_ref']) == S.V_REF
    assert np.array_equal(g['full'], H.smoothed_path(1, 1))
    assert g['state'][10:, 2].min() < 0.3 and g['state'][:, 2].max() > 5.0        # the ego slows to a crawl and goes on


def test_golden_replay_on_the_oracle():
    """every step of the recorded run from the recorded state before it, the cars' recorded get() rows and the previous step's recorded
    solution as warm start: traj_agent_idx, hit, stop index, target_ind and reaches_end identical, xref bit-identical (xref[2] = the speed
    profile with its zeros), controls within 1e-9"""
    g = H.gold('closedloop_speedref.npz')
    full = g['full']
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    centers, radius = _car()
    margin = 4 * int(np.ceil(radius / dl))
    p = S.speed_params(13)
    tidx = target = 0
    worst = 0.0
    n_zero = 0
    for i in range(int(g['steps'])):
        uw = None if i == 0 else np.stack([g['oa'][i - 1], g['od'][i - 1]])
        r = S.agent_step(p, full, dl, g['state'][i], g['obs6'][i], tidx, 0 if i == 0 else len(full), target, uw, centers, radius, margin)
        hit = -1 if r['hit'] is None else int(r['hit'][2])
        assert (r['traj_idx'], hit, r['stop'], r['target_ind']) == (g['tidx'][i], g['hit'][i][2], g['stop'][i], g['target'][i]), i
        assert np.array_equal(r['re'], g['re'][i]), i
        assert np.array_equal(r['xref'], g['xref'][i]), i
        assert r['sol'].status == 0 == g['status'][i]
        du = max(abs(r['sol'].u[1, 0] - g['ctrl'][i][0]), abs(r['sol'].u[0, 0] - g['ctrl'][i][1]),
                 float(np.abs(r['sol'].u - np.stack([g['oa'][i], g['od'][i]])).max()))
        worst = max(worst, du)
        n_zero += bool((r['xref'][2] == 0).any() and (r['xref'][2] == S.V_REF).any())
        tidx, target = r['traj_idx'], r['target_ind']
    print('speed-reference golden on the oracle: worst |control - golden| %.2e, %d steps with the stop index inside the window' % (worst, n_zero))
    assert worst < CTRL_TOL, worst
    assert n_zero >= 10


def test_stop_index_999_on_a_long_path_is_no_stop():
    """a straight path of 1500 points, the ego at point 890 and a standing car across the path, moved along it point by point until the
    conflict search's cut index is exactly 999 -- and lib/mpc_with_speed.py:281 (`if cutoff_idx != 999`) zeroes nothing.  One point further it does."""
    dl = 0.05
    n = 1500
    full = np.column_stack([np.arange(n) * dl, np.zeros(n), np.zeros(n)])
    centers, radius = _car()
    margin = 4 * int(np.ceil(radius / dl))
    p = S.speed_params(13)
    state = [full[890, 0], 0.0, 6.0, 0.0]
    seen = {}
    for shift in range(0, 400):
        obs = np.array([[full[1000 + shift, 0], 0.0, 0.0, np.pi / 2, 0.0, 0.0]])
        r = S.agent_step(p, full, dl, state, obs, 890, n, 890, None, centers, radius, margin)
        if r['hit'] is not None:
            seen[r['stop']] = r
        if 999 in seen and 1000 in seen:
            break
    assert 999 in seen and 1000 in seen, sorted(seen)
    quirk, plain = seen[999], seen[1000]
    assert quirk['hit'] is not None and (quirk['xref'][2] == S.V_REF).all()           # a real conflict, and no zeroing
    idx = np.minimum(np.rint(np.cumsum(np.full(14, 6.0 * 0.2)) / dl).astype(int) + quirk['target_ind'], n - 1)
    assert idx.max() >= 1000 and idx.min() < 999                                      # ... although the window reaches past index 999
    assert np.array_equal(plain['xref'][2], np.where(idx >= 1000, 0.0, S.V_REF))
    assert (plain['xref'][2] == 0).any() and (plain['xref'][2] == S.V_REF).any()
    # the profile rule itself
    assert (S.speed_profile(n, 999) == S.V_REF).all() and (S.speed_profile(n, 998)[998:] == 0).all() and (S.speed_profile(n, 998)[:998] == S.V_REF).all()
