"""Keep clear (mpcx_keepclear) without a GPU: the host build of the rule (csrc/mpcx_keepclear_core.h through
tests/keepclear_ref/keepclear_ref.cpp; keepclear_kernel compiles the very same header) against a numpy restatement on hand-made junctions,
the same program under the sanitizers, cross_phase_conflicts() on the stock routes, the rule on the CPU oracle -- the late-straight scene:
without the rule the first car of a phase enters an occupied box, with it nobody does --, the ctypes mirror and the new file's kernels.
The device side is tests/test_gpu_keepclear.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import keepclear_helpers as KH
from tests.test_precedence_cpu import _usage

ROOT = os.path.dirname(KH.HERE)
SIZES = (1, 3, 8, 64)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return KH.build_ref(tmp_path_factory.mktemp('keepclear_ref'))


@pytest.mark.parametrize('n_per', SIZES)
def test_rule_on_hand_made_junctions(ref, n_per):
    """K1.  keepclear_helpers.CASES (and WIDE at n_per = 64), one junction per case with the expected words beside it, at n_per = 1, 3, 8
    and 64.  The host build walking the junctions forwards and backwards and the numpy restatement give identical cut_len, boxed, waited,
    occupied and n_boxed, byte for byte, with and without the retirement words, and they are the values written down by hand; nothing
    else is written.  The cases: every OUT reason, INSIDE with and without a line, APPROACH outside the detector, a candidate that waited,
    one that can stop, one that cannot, one exactly on the stopping distance, a signal-held agent, a conflicting movement inside the
    junction before (no leak), a same-lane movement inside, a conflict cut shorter than the line."""
    w, want = KH.hand_made(n_per)
    fwd, bwd, twin, twin_b = (KH.copy_words(w) for _ in range(4))
    log = []
    n = [KH.host_rule(ref, fwd), KH.host_rule(ref, bwd, backwards=True), KH.rule_numpy(twin, log=log), KH.rule_numpy(twin_b, backwards=True)]
    assert len(set(n)) == 1 and n[0] == sum(1 for v in want[2].values() if v[0]) == int(want[1].sum()), n
    for k in KH.OUT_KEYS:
        assert fwd[k].tobytes() == bwd[k].tobytes() == twin[k].tobytes() == twin_b[k].tobytes() and fwd[k].dtype == np.int32, k
    KH.check_against_want(fwd, want, w)
    J = len(w['occupied'])
    assert J == sum(1 for c in KH.CASES if len(c[1]) <= n_per) + (len(KH.WIDE) if n_per == 64 else 0) and (n_per < 3 or J >= len(KH.CASES))
    for k in w:         # nothing else is written
        if k not in KH.OUT_KEYS and isinstance(w[k], np.ndarray):
            assert fwd[k].tobytes() == w[k].tobytes(), k
    if n_per >= 3:
        assert {why for *_, why in log} == {'waited', 'can stop', 'exempt'}
        assert sorted(set(fwd['boxed'].tolist())) == [0, 1] and (fwd['waited'] != w['waited']).any() and (fwd['cut_len'] != w['cut_len']).any()
        # without the retirement words the done car inside occupies, and the done candidate is boxed
        free = KH.copy_words(w); free['done'] = None
        twin = KH.copy_words(free)
        assert KH.host_rule(ref, free) == KH.rule_numpy(twin) == n[0] + 2
        assert all(free[k].tobytes() == twin[k].tobytes() for k in KH.OUT_KEYS)
        j = next(i for i, c in enumerate(KH.CASES) if c[0].startswith('OUT: done inside'))
        assert (free['occupied'][j], free['n_boxed'][j]) == (4, 1) and (fwd['occupied'][j], fwd['n_boxed'][j]) == (0, 0)
    if n_per == 64:
        assert fwd['n_boxed'][-3:].tolist() == [63, 0, 31] and fwd['occupied'][-3:].tolist() == [4, 0, 8]


@pytest.mark.parametrize('seed', range(4))
def test_rule_on_random_words(ref, seed):
    """K1.  seeded random junctions on the same tables (n_per 3 and 8): host build = numpy restatement, byte for byte, forwards and backwards"""
    for n_per, J in ((3, 40), (8, 33)):
        w = KH.random_words(seed, n_per, J)
        a, b, t = (KH.copy_words(w) for _ in range(3))
        assert KH.host_rule(ref, a) == KH.host_rule(ref, b, backwards=True) == KH.rule_numpy(t)
        assert all(a[k].tobytes() == b[k].tobytes() == t[k].tobytes() for k in KH.OUT_KEYS)
        assert a['boxed'].any() and a['occupied'].any() and (a['waited'] != w['waited']).any()


def test_host_build_under_sanitizers(ref, tmp_path):
    """K2.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on K1's
    junctions at every size, forwards and backwards, with and without the retirement words, on random words and on an empty case: no
    report, and the bytes of the plain build"""
    exe = str(tmp_path / 'keepclear_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DKEEPCLEAR_REF_MAIN'] + KH.INC + ['-o', exe, KH.SRC], check=True)
    blob, want = b'', b''
    cases = []
    for n_per in SIZES:
        for back in (0, 1):
            for with_done in (True, False):
                w, _ = KH.hand_made(n_per)
                if not with_done:
                    w['done'] = None
                cases.append((w, back))
    cases.append((KH.random_words(7, 8, 33), 0))
    for w, back in cases:
        blob += KH.blob(w, back)
        want += KH.out_bytes(w, KH.host_rule(ref, w, backwards=bool(back)))
    w, _ = KH.hand_made(3)
    empty = KH.words(**{k: (v[:0] if k in KH.PER_AGENT + KH.PER_JUNCTION else v) for k, v in w.items()})
    blob += KH.blob(empty, 0)
    want += np.array([0], np.int32).tobytes()
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert open(outp, 'rb').read() == want and len(want) > 4 * 4 * 3 * 17


# the pairs of movements DESIGN.md section 7 item 8 names, as (arm, exit arm) > (arm, exit arm)
NAMED = (((3, 1), (4, 2)), ((2, 4), (3, 1)), ((1, 3), (2, 4)), ((1, 2), (2, 4)), ((1, 3), (4, 1)), ((1, 2), (4, 1)), ((2, 3), (3, 4)), ((3, 4), (4, 1)))


def _movement(arm, out):
    """3 (arm - 1) + (turn - 1) of the movement from `arm` to the arm `out` (arms 1 .. 4, clockwise seen from above)"""
    return 3 * (arm - 1) + ((out - arm) % 4) - 1


def test_cross_phase_conflicts_of_the_stock_routes():
    """K3.  cross_phase_conflicts() on movement_conflicts() of the twelve stock routes: symmetric, no diagonal, a subset of the full table;
    no pair of arms {1, 3} or of arms {2, 4} survives (a permissive turn is not blocked by the opposed arm) and every cross-phase pair of the
    full table does; the eight pairs named in DESIGN.md section 7 item 8 survive; other phases give other tables."""
    from mpc_for_av_at_intersection_amd.batch import cross_phase_conflicts, movement_conflicts, movement_lines
    pairs = [(sp, ti) for sp in (1, 2, 3, 4) for ti in (1, 2, 3)]
    routes = [H.smoothed_path(sp, ti) for sp, ti in pairs]
    stop, group, ex = movement_lines(routes)
    full, _ = movement_conflicts(routes, stop, ex, [2.18, 0.68], np.sqrt(2.0))
    cross = cross_phase_conflicts(full)
    assert cross.dtype == np.int32 and cross.shape == (12,)
    bit = lambda tab, g, h: (int(tab[g]) >> h) & 1
    same = lambda g, h: (g // 3) % 2 == (h // 3) % 2
    for g in range(12):
        assert not bit(cross, g, g)
        for h in range(12):
            assert bit(cross, g, h) == bit(cross, h, g)
            assert bit(cross, g, h) == (bit(full, g, h) and not same(g, h)), (g, h)
    assert 0 < sum(bin(int(c)).count('1') for c in cross) < sum(bin(int(c)).count('1') for c in full)
    for (a, ao), (b, bo) in NAMED:
        g, h = _movement(a, ao), _movement(b, bo)
        assert bit(cross, g, h) and bit(cross, h, g), ((a, ao), (b, bo), g, h)
    assert _movement(1, 3) == 1 and _movement(2, 4) == 4 and _movement(1, 2) == 0 and _movement(4, 1) == 9
    # one phase for all: nothing is left; one phase per arm: everything is
    assert not cross_phase_conflicts(full, phases=((0, 1, 2, 3),)).any()
    assert np.array_equal(cross_phase_conflicts(full, phases=((0,), (1,), (2,), (3,))), full)
    # the tables of the batch's default: the pair of the late-straight scene
    assert bit(cross, 1, 4)


@pytest.fixture(scope='module')
def late_runs():
    """the oracle runs of K4, computed once: (stop mode, rule on) under the plan, and the cut-mode pair under the controller"""
    from mpc_for_av_at_intersection_amd.batch import two_phase_controller
    runs = {}
    for speed in (False, True):
        for on in (False, True):
            loop = KH.late_loop(on, speed=speed)
            runs[speed, on] = (loop, loop.run(200))
    ct = two_phase_controller(detect=max(int(s[0]) for s in KH.late_tables()[3]), **KH.LATE_CONTROLLER)
    for on in (False, True):
        loop = KH.late_loop(on, controller=ct)
        runs['actuated', on] = (loop, loop.run(200))
    return runs


@pytest.mark.parametrize('mode', [False, True, 'actuated'], ids=['cut', 'speed', 'actuated'])
def test_late_straight_on_the_oracle(late_runs, mode):
    """K4.  The late straight (keepclear_helpers: one straight from arm 1, one from arm 2, a two-phase plan without all-red; T = 13) on the
    CPU oracle, in both stop modes under the plan and in cut mode under two_phase_controller.  An ENTRY INTO AN OCCUPIED BOX is a step in
    which an agent's traj_idx passes its stop line while occ of that step holds a movement that conflicts with its own.  The condition on
    the inputs first: without the rule the scene has such an entry.  With the rule it has none, and no candidate of the run takes the
    cannot-stop exemption (the rule's guarantee is about cars that can stop).  Both cars arrive; the worst clearance with the rule is
    positive and not below the run without it; the arm-2 car is boxed in at least one step and the arm-1 car never.  In speed mode the
    hold is soft (a boxed car creeps on at about 0.5 m/s), so the scene there is the last steps of the crossing: see keepclear_helpers."""
    off, _ = late_runs[mode, False]
    on, hist = late_runs[mode, True]
    exempt = [c for c in on.candidates if c[4] == 'exempt']
    print('late straight, %s: entries without %s, with %s; boxed steps %s; exempt %d; arrivals %s -> %s; worst clearance %.2f -> %.2f m'
          % (mode, off.entries, on.entries, on.boxed_steps.tolist(), len(exempt), off.arrival, on.arrival, off.worst_clearance, on.worst_clearance))
    assert len(off.entries) >= 1 and all(a == 1 for _, a in off.entries), off.entries        # the condition on the inputs
    assert on.entries == []
    assert exempt == []
    assert all(on.done) and all(off.done) and 0 < max(on.arrival) <= 200
    assert on.worst_clearance > 0.0 and on.worst_clearance >= off.worst_clearance
    assert on.boxed_steps[1] >= 1 and on.boxed_steps[0] == 0 and not off.boxed_steps.any()
    assert {c[4] for c in on.candidates} == {'waited'} and all(c[1] == 1 for c in on.candidates)
    # the box the arm-2 car waited for is the arm-1 car's movement, and it passes its line only when that movement has left
    first = next(s for s, h in enumerate(hist) if h[1] is not None and h[1]['traj_idx'] >= on.line[1])
    assert all(o == 2 for o in on.occ_hist[on.candidates[0][0]:on.candidates[-1][0] + 1]) and not on.occ_hist[first] & 2
    assert first > off.entries[0][0]


def test_struct_mirror_matches_the_header(ref):
    """K5.  _lib.KeepClearC against the layout the header's own compiler gives mpcx_keepclear and the field names parsed from the header;
    the junction limit agrees with _lib; the new exports are there; every older struct keeps its size"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 32)()
    ref.keepclear_ref_layout(lay)
    names = [n for n, _ in _lib.KeepClearC._fields_]
    assert names == ['path_move', 'path_exit', 'conflict', 'boxed', 'waited', 'occupied', 'n_boxed', 'detect', 'n_per', 'n_junctions', 'n_moves',
                     'n_points', 'reserved']
    assert C.sizeof(_lib.KeepClearC) == 80
    assert list(lay)[:14] == [C.sizeof(_lib.KeepClearC)] + [getattr(_lib.KeepClearC, n).offset for n in names]
    assert lay[14] == _lib.KEEPCLEAR_PER_MAX == 64
    assert list(lay)[15:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC),
                              C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC), C.sizeof(_lib.RespawnC), C.sizeof(_lib.RoutesC),
                              C.sizeof(_lib.PrecedenceC), C.sizeof(_lib.SignalsC), C.sizeof(_lib.ActuationC), C.sizeof(_lib.AdviceC),
                              C.sizeof(_lib.IntentC), C.sizeof(_lib.ReservationC), C.sizeof(_lib.FollowingC), C.sizeof(_lib.SafetyC),
                              C.sizeof(_lib.SightC)]
    assert list(lay)[16:28] == [24, 80, 32, 16, 40, 56, 64, 24, 88, 80, 40, 24] and lay[28] == 96        # as tests/test_reserve_cpu.py has them
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_keepclear;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_set_keepclear', 'mpcx_keepclear_step_batch'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_keepclear_kernels_need_no_scratch():
    """K6.  mpcx_keepclear.hip cross-compiled for gfx950 with the Makefile's flags: exactly the seven lane-group instantiations of its one
    kernel (G = 1 .. 64), none with scratch, spills or LDS"""
    use = _usage('mpcx_keepclear.hip')
    assert len(use) == 7 and all('keepclear_kernel' in k for k in use), sorted(use)
    assert sorted(int(re.search(r'keepclear_kernelILi(\d+)E', k).group(1)) for k in use) == [1, 2, 4, 8, 16, 32, 64]
    for name, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (name, u)
