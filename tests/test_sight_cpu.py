"""Line of sight on the CPU (no GPU): the host build of csrc/mpcx_sight_core.h forwards and backwards, the numpy restatement and words
written down by hand agree byte for byte; the stock world with corner_blocks(); 60 seeded scenes; the stand-alone program under the
sanitizers; the ctypes mirror of mpcx_sight; two cars at a blind corner on the CPU oracle."""
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import sight_helpers as ST


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return ST.build_ref(tmp_path_factory.mktemp('sight_ref'))


def _all_three(ref, w, what):
    fwd, back, npy = ST.host_step(ref, w), ST.host_step(ref, w, backwards=True), ST.rule_numpy(w)
    ST.same(fwd, back, what + ': host forwards vs backwards')
    ST.same(fwd, npy, what + ': host vs numpy')
    return fwd


def test_hand_made_probes(ref):
    """S1.  one agent and one other per probe, geometry exact in binary (sight_helpers.PROBES: range exactly met and one ulp beyond,
    parallel to an edge outside / inside / along it, the grazed corner, eye or target inside, T == E inside and outside, the culled occluder,
    the octagon, the empty set, a set word outside the table, two occluders in a set, heard rows in and out of range): host forwards =
    host backwards = numpy = the values written down"""
    n = 0
    for w, exp in ST.probe_words():
        ST.same(_all_three(ref, w, 'probes at range %g' % w['range']), exp, 'probes at range %g vs by hand' % w['range'])
        n += len(exp[0])
    assert n == len(ST.PROBES)


def test_shrink_turns_a_hidden_row_seen(ref):
    """S2.  y = 3.75 crosses the square [2, 4]^2 and passes over the same square shrunk by 1/2 (occluder_table(shrink=0.5))"""
    (w0, exp0), = ST.probe_words([ST.PROBES[-1]], [[ST.box_a()]])
    assert exp0[0].tolist() == [0]
    ST.same(_all_three(ref, w0, 'unshrunk'), exp0, 'unshrunk vs by hand')
    w1, exp1 = ST.shrunk_probe()
    assert w1['box'].tolist() == [[2.5, 2.5, 3.5, 3.5]]
    ST.same(_all_three(ref, w1, 'shrunk'), exp1, 'shrunk vs by hand')


def test_windows_own_rows_absent_and_retired(ref):
    """S3.  nobody else, windows of 1, 16, 17, 64 and 70 rows, the own row inside, below, above the pool and missing, a window that runs past
    either end of the pool, an empty and a negative count, a retired agent; then the same with row 1 absent"""
    for (w, exp), what in zip(ST.window_words(), ('no scene', 'row 1 absent')):
        ST.same(_all_three(ref, w, what), exp, what + ' vs by hand')
    # nobody else: a pool of the agent's own row alone
    w = dict(w, state=np.zeros((1, 4)), obs6=np.zeros((1, 6)), obs_off=[0], obs_cnt=[1], obs_skip=[0], set_of=[0], done=None, absent=None)
    ST.same(_all_three(ref, w, 'alone'), (np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.int32)), 'alone')


def test_two_sets_in_one_call(ref):
    """S4.  the same pair of cars behind the square for one agent and at an open junction for the other, in one call"""
    p = [((0.0, 0.0), (6.0, 6.0), 0, 0, 32.0, False), ((0.0, 0.0), (6.0, 6.0), 2, 0, 32.0, True)]
    (w, exp), = ST.probe_words(p)
    assert exp[0].tolist() == [0, 2]
    ST.same(_all_three(ref, w, 'two sets'), exp, 'two sets vs by hand')


def test_stock_world_corner_blocks(ref):
    """S5.  the stock four-way world with corner_blocks(5): a car at (3, -20) on the southern arm does not see one at (-20, -3) on the
    western arm, from (3, -6) it does; along the stock south -> west route the other car comes into view at one path index and stays"""
    from mpc_for_av_at_intersection_amd.batch import corner_blocks

    def sees(eye, target):
        w = dict(state=[[eye[0], eye[1], 0, 0]], obs6=[[eye[0], eye[1], 0, 0, 0, 0], [target[0], target[1], 0, 0, 0, 0]], obs_off=[0],
                 obs_cnt=[2], obs_skip=[0], set_of=[0], done=None, absent=None, heard=None, range=60.0, **ST.tables([corner_blocks(5.0)]))
        return int(_all_three(ref, w, 'stock world')[0][0]) == 2
    assert not sees((3.0, -20.0), (-20.0, -3.0))
    assert sees((3.0, -6.0), (-20.0, -3.0))
    path = H.smoothed_path(*SOUTH_TO_WEST)
    assert path[0, 1] < -29 and abs(path[0, 0] - 3.0) < 0.5 and path[-1, 0] < -29, 'the route enters from the south and leaves to the west'
    seen = [sees((float(x), float(y)), (-20.0, -3.0)) for x, y in path[:, :2]]
    first = seen.index(True)
    print('first index of the south -> west route that sees (-20, -3):', first, path[first, :2])
    assert first == FIRST_SEEN_INDEX and all(seen[first:]) and not any(seen[:first])


def test_seeded_scenes(ref):
    """S6.  60 seeded scenes, P in {5, 17, 33}, up to 24 occluders in three sets: host forwards = backwards = numpy, byte for byte, and
    every scene has both seen and hidden rows"""
    sizes = set()
    for seed in range(60):
        w = ST.random_words(seed)
        got = _all_three(ref, w, 'seed %d' % seed)
        assert got[1].sum() > 0 and got[2].sum() > 0, 'seed %d: %d seen, %d hidden' % (seed, got[1].sum(), got[2].sum())
        assert (got[1] + got[2] <= len(w['obs6']) - 1).all()
        sizes.add(len(w['state']))
    assert sizes == {5, 17, 33}


def test_host_build_under_sanitizers(ref, tmp_path):
    """S7.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on the
    hand-made and the seeded words, forwards and backwards, and on an empty case: no report, and the words are the shared library's"""
    exe = ST.build_main(tmp_path, sanitize=True)
    words = [w for w, _ in ST.probe_words()] + [w for w, _ in ST.window_words()] + [ST.shrunk_probe()[0]] + [ST.random_words(s) for s in range(60)]
    empty = dict(ST.shrunk_probe()[0], state=np.zeros((0, 4)), obs6=np.zeros((0, 6)), obs_off=[], obs_cnt=[], obs_skip=[], set_of=[], heard=None)
    cases = [(w, back) for w in words for back in (0, 1)] + [(empty, 0)]
    fin, fout = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    ST.write_cases(fin, cases)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    for (w, back), got in zip(cases, ST.read_results(fout, cases)):
        if len(got[0]):
            ST.same(got, ST.host_step(ref, w, backwards=bool(back)), 'sanitized program')


def test_ctypes_mirror(tmp_path):
    """S8.  _lib.SightC has the size and the field offsets of mpcx_sight as the header's own compiler lays it out (the stand-alone
    program's printout)"""
    from mpc_for_av_at_intersection_amd import _lib
    exe = ST.build_main(tmp_path)
    out = subprocess.run([exe, '--layout'], capture_output=True, text=True, check=True).stdout.split()
    want = [int(v) for v in out]
    assert len(want) == 16 and [n for n, _ in _lib.SightC._fields_] == list(ST.FIELDS)
    assert [C_sizeof(_lib.SightC)] + [getattr(_lib.SightC, n).offset for n in ST.FIELDS] == want


def test_kernels_need_no_scratch():
    """S10.  mpcx_sight.hip cross-compiled for gfx950 with the Makefile's flags: exactly its one kernel, no scratch, no spills, no LDS;
    mpcx_interaction_sight.hip holds exactly the two line-of-sight kernels of the conflict search, which keep five wavefronts per SIMD
    within 96 VGPRs without scratch or static LDS, as the kernels they are made from"""
    from tests.test_precedence_cpu import _usage
    use = _usage('mpcx_sight.hip')
    assert len(use) == 1 and 'sight_kernel' in next(iter(use)), sorted(use)
    u = next(iter(use.values()))
    assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, u
    use = _usage('mpcx_interaction_sight.hip')
    assert len(use) == 2 and all('interaction_sight_kernelILb%dEE' % k in ''.join(use) for k in (0, 1)), sorted(use)
    for n, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (n, u)
        assert u['VGPRs'] <= 96 and u['Occupancy [waves/SIMD]'] == 5, (n, u)


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def _first_cut(loop, n, agent=0):
    """the first step (0-based) in which `agent` has a conflict cut, -1 = none within n steps"""
    for s in range(n):
        out = loop.step()
        if out[agent] is not None and out[agent]['hit'] >= 0:
            return s
    return -1


def test_blind_corner_on_the_oracle():
    """S9.  two cars on perpendicular arms of the stock world on the CPU oracle, T = 13: car 0 from the south, car 1 from the west, both
    straight on.  At the open junction car 0 first cuts its path for car 1 in step OPEN_STEP; with corner_blocks() the first cut comes
    later, in step BLIND_STEP, because until then the building hides car 1; when car 1 is heard (a connected vehicle) it is the open
    junction's step again."""
    from mpc_for_av_at_intersection_amd.batch import corner_blocks
    paths, dl, start = blind_corner_setup()

    def loop(**kw):
        return ST.SightOracleLoop(paths, dl, start, mode='all', T=13, depart=True, **kw)
    open_step = _first_cut(loop(), 40)
    blind = loop(obstacles=corner_blocks())
    blind_step = _first_cut(blind, 40)
    heard_step = _first_cut(loop(obstacles=corner_blocks(), heard=np.array([0, 1], np.int32)), 40)
    print('first conflict cut of car 0: open', open_step, 'blind', blind_step, 'heard', heard_step)
    assert (open_step, blind_step, heard_step) == (OPEN_STEP, BLIND_STEP, OPEN_STEP) and 0 <= OPEN_STEP < BLIND_STEP
    # until the cut car 0 did not see car 1 in the blind run
    assert all(int(w[0][0]) == 0 for w in blind.sight_hist[:BLIND_STEP]) and int(blind.sight_hist[BLIND_STEP][0][0]) == 2


SOUTH_TO_WEST = (1, 1)      # H.smoothed_path(arm, turn) of the stock route from the southern arm to the western
FIRST_SEEN_INDEX = 295      # (1.085, -5.810): the sight line to (-20, -3) clears the corner (-5, -5) of the south-western block
OPEN_STEP, BLIND_STEP = 1, 24       # from the oracle run (printed by the test)


def blind_corner_setup():
    """the straight routes from the south and from the west and start indices some 30 m before the crossing"""
    paths = [H.smoothed_path(*pr) for pr in BLIND_PAIRS]
    dl = float(np.linalg.norm(paths[0][0, :2] - paths[0][1, :2]))
    return paths, dl, list(BLIND_START)


BLIND_PAIRS = ((1, 2), (2, 2))
BLIND_START = (0, 0)
