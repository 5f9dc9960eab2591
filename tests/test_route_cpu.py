"""Routes (mpcx_routes: every vehicle of a respawning slot takes its own route from its own start pose) without a GPU: the host build of
csrc/mpcx_route_core.h (tests/route_ref/route_ref.cpp; respawn_route_kernel and summary_kernel compile the very same header) against a
numpy restatement on hand-made words, the rule inside the closed loop on the CPU oracle, the sanitizers, the ctypes mirror, the kernels'
resource usage, batch.turning_demand and the per-movement summary.  The device side is tests/test_gpu_route.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import admit_helpers as AH
from tests import helpers as H
from tests import respawn_helpers as RH
from tests import route_helpers as TH

ROOT = RH.ROOT
CASES = [(True, False), (False, False), (True, True), (False, True)]


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return TH.build_ref(tmp_path_factory.mktemp('route_ref'))


@pytest.fixture(scope='module')
def respawn_ref(tmp_path_factory):
    return RH.build_ref(tmp_path_factory.mktemp('respawn_ref'))


@pytest.fixture(scope='module')
def admit_ref(tmp_path_factory):
    return AH.build_ref(tmp_path_factory.mktemp('admit_ref'))


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in TH.MUT_F64 + TH.MUT_I32)


@pytest.mark.parametrize('log,speed', CASES)
def test_rule_on_hand_made_words(ref, respawn_ref, log, speed):
    """R1.  Nine agents (route_helpers.hand_made), with and without log words and with prev_len.  The host build visiting the lanes
    forwards and backwards and the numpy restatement give identical words, byte for byte.  Agents that did not arrive are untouched.  A reset
    slot (2, 3) holds its next vehicle's start pose, start index, route offset and route length; word 7 of every new record is the
    episode's route.  The last vehicle of a slot (4) leaves path_off and path_len alone.  A slot whose next route index is R (5) or whose
    next start index is route_len (6) ends never driven: wait = entered_step = -1, done set, path_off and path_len unchanged -- and a
    second step finds nobody arrived.  With the route word excluded, every word of every agent but the two defective ones -- and every
    word but wait and entered_step of those -- equals what the respawn rule alone (tests/respawn_ref) produces, state, traj_idx and
    target_ind of the reset slots apart."""
    case = TH.hand_made(log, speed)
    before = case.words()
    fwd, bwd, twin, plain = case.copy(), case.copy(), case.copy(), case.plain()
    n = len(TH.ARRIVE)
    assert TH.host_step(ref, fwd) == n and TH.host_step(ref, bwd, backwards=True) == n and TH.numpy_step(twin) == TH.ARRIVE
    after = fwd.words()
    assert _same(after, bwd.words()) and _same(after, twin.words())
    untouched = [q for q in range(case.P) if q not in TH.ARRIVE]
    for k in before:
        assert before[k][untouched].tobytes() == after[k][untouched].tobytes(), k
    G = case.G
    for q in TH.ARRIVE:
        g = int(case.served[q])
        assert after['served'][q] == g + 1 and after['ep_i32'][q, g, 7] == case.route_of[q, g]
        assert after['ep_i32'][q, g, 0] == case.entered[q] and after['ep_i32'][q, g, 1] == 19
    for q in TH.RESET:
        g1 = int(case.served[q]) + 1
        r = int(case.route_of[q, g1])
        assert np.array_equal(after['state'][q], case.rstart_state[q, g1]) and not np.array_equal(after['state'][q], case.start_state[q])
        assert after['traj_idx'][q] == after['target_ind'][q] == case.rstart_idx[q, g1]
        assert after['path_off'][q] == case.route_off[r] != before['path_off'][q] and after['path_len'][q] == case.route_len[r]
        assert after['wait'][q] >= 0 and after['entered'][q] == -1
    assert (after['path_off'][2], after['path_len'][2]) == (1500, 650) and (after['path_off'][3], after['path_len'][3]) == (700, 800)
    for k in before:        # the last vehicle: its record and the count, nothing else -- path_off and path_len included
        if k not in ('served', 'ep_i32', 'ep_f64'):
            assert before[k][4].tobytes() == after[k][4].tobytes(), k
    for q in TH.DEFECT:
        assert after['wait'][q] == -1 and after['entered'][q] == -1 and case.done[q] == 1
        assert after['path_off'][q] == before['path_off'][q] and after['path_len'][q] == before['path_len'][q]
        assert after['traj_idx'][q] == case.start_idx[q]            # (what the plain reset wrote stays: nothing reads it)
    # against the respawn rule alone
    assert RH.host_step(respawn_ref, plain) == n
    alone = plain.words()
    for k in alone:
        got, want = after[k].copy(), alone[k].copy()
        if k == 'ep_i32':
            got[..., 7] = want[..., 7] = 0
        if k in ('state', 'traj_idx', 'target_ind'):
            got[TH.RESET] = want[TH.RESET] = 0
        if k in ('wait', 'entered'):
            assert (want[TH.DEFECT] != -1).all() if k == 'wait' else (want[TH.DEFECT] == -1).all()
            got[TH.DEFECT] = want[TH.DEFECT] = 0
        assert got.tobytes() == want.tobytes(), k
    fwd.clock[0] += 1
    assert TH.host_step(ref, fwd) == 0
    assert _same(after, fwd.words())


def test_larger_hand_made_case():
    """R1.  hand_made(P=65) repeats the nine agents: what the device test runs in two blocks"""
    c = TH.hand_made(True, True, P=65)
    assert c.P == 65 and c.state.shape == (65, 4) and c.route_of.shape == (65, 3) and c.own.tolist() == list(range(65))
    assert TH.numpy_step(c) == [q for q in range(65) if q % 9 in TH.ARRIVE]


def _routes12():
    return [H.smoothed_path(1, 1), H.smoothed_path(1, 2)]


@pytest.mark.parametrize('speed', [False, True])
def test_lone_slot_on_the_oracle(ref, respawn_ref, admit_ref, speed):
    """R2.  The rule inside the closed loop on the CPU oracle (T = 13, v0 = 0): one slot, G = 3, on the stock routes (1, 1), (1, 2),
    (1, 1), each from index len(route) - 120, due all 0, gap 0.  Every episode's steps_driven and every state along it equal those of an
    UNROUTED RespawnOracleLoop (one vehicle) on that route from that index -- compared against the existing loop, no recorded numbers --
    and episode 3 equals episode 1."""
    routes = _routes12()
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    order = [0, 1, 0]
    start = [len(routes[r]) - 120 for r in order]
    loop = TH.RouteOracleLoop(admit_ref, ref, routes, dl, [order], [start], due=[[0, 0, 0]], gap=0.0, T=13, speed=speed)
    hist = loop.run(200)
    eps = loop.episodes(0)
    print('lone slot, speed=%s: %s in %d steps' % (speed, eps, len(hist)))
    assert loop.served.tolist() == [3] and len(eps) == 3 and loop.ep_i32[0, :, 7].tolist() == order
    posts = []
    for g, (e, a, d) in enumerate(eps):
        assert d == a - e + 1
        posts.append(np.array([hist[s][0]['post'] for s in range(e, a + 1)]))
        alone = RH.RespawnOracleLoop(admit_ref, respawn_ref, [routes[order[g]]], dl, [start[g]], due=[[0]], gap=0.0, T=13, speed=speed)
        h = alone.run(200)
        (e1, a1, d1), = alone.episodes(0)
        assert (e1, d1) == (0, d) and len(h) == d
        assert np.array_equal(posts[g], np.array([s[0]['post'] for s in h])), g
    assert np.array_equal(posts[0], posts[2]) and not np.array_equal(posts[0][-1], posts[1][-1])
    assert loop.path_off.tolist() == [0] and loop.path_len.tolist() == [len(routes[0])]


def test_queue_on_the_oracle(ref, admit_ref):
    """R2.  Two slots at the FIRST point of arm 1 -- one start pose, one queue --, G = 2, routes [[0, 1], [1, 0]] of the stock routes
    (1, 1) and (1, 2), due all 0, gap 1 m, cut mode.  The two slots are never admitted in the same step; steps_driven == arrived - entered
    + 1 in every record; word 7 equals route_of.  Observed on the oracle when this test was written: the run takes 219 steps -- the
    episodes are (entered, arrived, driven) = (0, 99, 100), (100, 207, 108) and (13, 105, 93), (114, 218, 105) -- and the conflict search
    hits in 157 agent-steps."""
    routes = _routes12()
    dl = float(np.linalg.norm(routes[0][0, :2] - routes[0][1, :2]))
    assert np.array_equal(routes[0][0], routes[1][0])
    route_of = [[0, 1], [1, 0]]
    loop = TH.RouteOracleLoop(admit_ref, ref, routes, dl, route_of, [[0, 0], [0, 0]], due=[[0, 0], [0, 0]], gap=1.0, T=13)
    hist = loop.run(600)
    print('queue: %s / %s in %d steps, %d hits' % (loop.episodes(0), loop.episodes(1), len(hist), loop.hits))
    assert loop.served.tolist() == [2, 2] and len(hist) < 600
    assert loop.ep_i32[:, :, 7].tolist() == route_of
    entered = []
    for a in range(2):
        for e, arr, d in loop.episodes(a):
            assert d == arr - e + 1
            entered.append(e)
    assert len(set(entered)) == 4
    assert len(hist) == 219 and loop.hits == 157
    assert [loop.episodes(0), loop.episodes(1)] == [[(0, 99, 100), (100, 207, 108)], [(13, 105, 93), (114, 218, 105)]]


def test_host_build_under_sanitizers(ref, tmp_path):
    """R3.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on R1's
    cases, forwards and backwards, two steps each: no report, and the bytes of the plain build"""
    exe = str(tmp_path / 'route_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DROUTE_REF_MAIN'] + TH.INC + ['-o', exe, TH.SRC], check=True)
    blob, want = b'', b''
    for log, speed in CASES:
        for back in (0, 1):
            c = TH.hand_made(log, speed)
            blob += c.serialise(back, 2)
            for _ in range(2):
                got = TH.host_step(ref, c, backwards=bool(back))
                want += c.blob() + np.int32(got).tobytes()
                c.clock[0] += 1
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    san = open(outp, 'rb').read()
    assert san == want and len(san) > 8000


def test_struct_mirror_matches_the_header(ref):
    """R4.  _lib.RoutesC against the layout the header's own compiler gives mpcx_routes and the field names parsed from the header; the new
    exports are there; every older struct keeps its size (mpcx_respawn: 56 bytes, 8 fields) and the episode record's names their length"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 17)()
    ref.route_ref_layout(lay)
    names = [n for n, _ in _lib.RoutesC._fields_]
    assert C.sizeof(_lib.RoutesC) == 64 and len(names) == 9
    assert list(lay)[:10] == [C.sizeof(_lib.RoutesC)] + [getattr(_lib.RoutesC, n).offset for n in names]
    assert list(lay)[10:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC),
                              C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC), C.sizeof(_lib.RespawnC)]
    assert list(lay)[11:] == [24, 80, 32, 16, 40, 56] and len(_lib.RespawnC._fields_) == 8
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_routes;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_routes', 'mpcx_respawn_step_batch_routes', 'mpcx_episode_summary'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)
    assert len(_lib.EPISODE_I32) == 7 and len(_lib.EPISODE_F64) == 1 and _lib.EPISODE_ROUTE_WORD == 7
    from mpc_for_av_at_intersection_amd.batch import EPISODE_DTYPE, MOVEMENT_DTYPE
    assert len(EPISODE_DTYPE.names) == 11 and MOVEMENT_DTYPE == TH.SUMMARY_DTYPE


def test_route_kernels_need_no_scratch():
    """R4.  mpcx_route.hip cross-compiled for gfx950 with the Makefile's flags: exactly the two kernels, no scratch, no spills and no LDS;
    mpcx_respawn.hip keeps its one kernel"""
    mk = open(os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('-I$(ROOT)/include', RH.INC[0])
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (.*)$', mk, re.M).group(1).strip()
    assert os.path.exists(hipcc), 'no hipcc at %s (set HIPCC): the kernels cannot be cross-compiled for this check' % hipcc
    found = {}
    for name in ('mpcx_route.hip', 'mpcx_respawn.hip'):
        src = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', name)
        res = subprocess.run([hipcc] + flags.split() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-S', '-o', os.devnull, src],
                             check=True, capture_output=True, text=True)
        use, cur = found.setdefault(name, {}), None
        for k, v in re.findall(r'remark:\s+([A-Za-z ]+(?: \[[^\]]*\])?): (\S+) \[-Rpass-analysis', res.stderr):
            if k == 'Function Name':
                cur = use.setdefault(v, {})
            elif cur is not None:
                cur[k.strip()] = int(v) if v.isdigit() else v
    print(found)
    use = found['mpcx_route.hip']
    assert len(use) == 2 and any('respawn_route_kernel' in n for n in use) and any('summary_kernel' in n for n in use), sorted(use)
    for n, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (n, u)
    assert len(found['mpcx_respawn.hip']) == 1


def _arms(n_arms=4, per_arm=2, n=6):
    """n_arms arms with per_arm routes each: the routes of an arm share their first point, pose and all"""
    routes = []
    for k in range(n_arms):
        first = np.array([10.0 * k, -30.0, 0.5 * k])
        for m in range(per_arm):
            tail = np.column_stack([10.0 * k + np.arange(1, n), -30.0 + (m + 1) * np.arange(1, n), np.full(n - 1, 0.5 * k)])
            routes.append(np.concatenate([first[None], tail]))
    return routes


def test_turning_demand():
    """R5.  batch.turning_demand: (B, A, G), deterministic per seed; every vehicle's route is one of its slot's arm; share [1, 0] per arm
    gives all the first route of the arm; a slot off the shared point has a single candidate and makes no draw (the stream of the others
    does not move); over 4096 draws the shares are within 3 sqrt(p (1 - p) / n) of the weights; bad input raises ValueError"""
    from mpc_for_av_at_intersection_amd.batch import turning_demand
    routes = _arms()
    B, A, G = 3, 8, 5
    route_of_agent = np.tile(np.arange(A), (B, 1))
    start = np.zeros((B, A), dtype=np.int64)
    share = np.array([3, 1, 1, 1, 1, 3, 0.5, 0.5])
    d = turning_demand(route_of_agent, routes, start, share, G, seed=3)
    assert d.shape == (B, A, G) and np.issubdtype(d.dtype, np.integer)
    assert np.array_equal(d, turning_demand(route_of_agent, routes, start, share, G, seed=3))
    assert not np.array_equal(d, turning_demand(route_of_agent, routes, start, share, G, seed=4))
    assert (d // 2 == (route_of_agent // 2)[:, :, None]).all()         # candidates stay within the arm
    rng = np.random.default_rng(3)                                      # the draws replay: instance-major, slot-major, G at once
    for b in range(B):
        for a in range(A):
            arm = [2 * (a // 2), 2 * (a // 2) + 1]
            w = share[arm] / share[arm].sum()
            assert d[b, a].tolist() == [arm[i] for i in rng.choice(2, size=G, p=w)]
    first = turning_demand(route_of_agent, routes, start, [1, 0] * 4, G, seed=5)
    assert (first == (2 * (route_of_agent // 2))[:, :, None]).all()
    off = start.copy()
    off[1, 3] = 2           # this slot starts down its own route: no other route passes there -> a single candidate, no draw
    e = turning_demand(route_of_agent, routes, off, share, G, seed=3)
    assert (e[1, 3] == 3).all()
    rng = np.random.default_rng(3)
    for b in range(B):
        for a in range(A):
            if (b, a) == (1, 3):
                continue
            arm = [2 * (a // 2), 2 * (a // 2) + 1]
            assert e[b, a].tolist() == [arm[i] for i in rng.choice(2, size=G, p=share[arm] / share[arm].sum())]
    n = 4096
    big = turning_demand(np.zeros((1, 1), dtype=np.int64), routes[:2], np.zeros((1, 1), dtype=np.int64), [0.3, 0.7], n, seed=11)
    p = 0.3
    got = float((big == 0).mean())
    print('share of route 0 over %d draws: %.4f (weight %.1f, 3 sigma %.4f)' % (n, got, p, 3 * np.sqrt(p * (1 - p) / n)))
    assert big.shape == (1, 1, n) and abs(got - p) <= 3 * np.sqrt(p * (1 - p) / n)
    assert turning_demand(route_of_agent, routes, start, share, 1, seed=3).shape == (B, A, 1)
    for bad in (dict(start_index=start[:, :4]), dict(generations=0), dict(share=share[:4]), dict(share=-share), dict(share=[0, 0] + [1] * 6),
                dict(route_of_agent=route_of_agent + 1), dict(start_index=start + 6)):
        kw = dict(route_of_agent=route_of_agent, routes=routes, start_index=start, share=share, generations=G, seed=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            turning_demand(**kw)


def test_summary_on_a_hand_made_table(ref):
    """R6.  the per-movement summary restated in numpy (route_helpers.summary_numpy -- the definition tests/test_gpu_route.py uses) on a
    hand-made episode table, figure by figure, and the host build of the kernel's loop gives the same bytes; unfinished records and
    records whose word 7 is no route are in no row; an all-empty table gives zeros and +inf"""
    A, G, R = 2, 3, 3
    P = 4
    served = np.array([3, 1, 0, 2], np.int32)
    w = np.full((P, G, 8), -9, np.int32)
    f = np.full((P, G, 2), -9.0)

    def rec(q, g, entered, arrived, driven, contact, due, route, clear):
        w[q, g] = [entered, arrived, driven, -1, contact, 1, due, route]
        f[q, g] = [clear, 0.0]
    rec(0, 0, 4, 30, 27, -1, 1, 0, 0.5)
    rec(0, 1, 40, 70, 31, 12, 35, 2, -0.1)
    rec(0, 2, 80, 99, 20, -1, 80, 0, 0.25)
    rec(1, 0, 7, 31, 25, 3, 0, 2, 0.75)
    rec(1, 1, 50, 60, 11, 5, 45, 2, -5.0)       # not finished (served[1] == 1): in no row
    rec(3, 0, 2, 20, 19, -1, 2, 1, np.inf)
    rec(3, 1, 30, 41, 12, -1, 22, 7, 0.01)      # word 7 is no route: in no row
    want = np.zeros((2, R), TH.SUMMARY_DTYPE)
    want['min_clearance'] = np.inf
    want[0, 0] = (2, 0, 3 + 0, 27 + 20, 0.25)
    want[0, 2] = (2, 2, 5 + 7, 31 + 25, -0.1)
    want[1, 1] = (1, 0, 0, 19, np.inf)
    got = TH.summary_numpy(A, R, served, w, f)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert TH.host_summary(ref, A, R, served, w, f).tobytes() == want.tobytes()
    empty = TH.summary_numpy(A, R, np.zeros(P, np.int32), w, f)
    assert not empty['count'].any() and not empty['delay_sum'].any() and np.isinf(empty['min_clearance']).all()
    assert TH.host_summary(ref, A, R, np.zeros(P, np.int32), w, f).tobytes() == empty.tobytes()
