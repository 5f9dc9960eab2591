"""Stop signs (mpcx_stopsign) without a GPU: the host build of the rule (csrc/mpcx_stopsign_core.h through
tests/stopsign_ref/stopsign_ref.cpp; stopsign_kernel compiles the very same header) against a plain-Python restatement of the seven steps
on seeded random junctions over three consecutive steps and on hand-made junctions, the ctypes mirror, sign_table() and the new file's
kernels.  The device side is tests/test_gpu_stopsign.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import stopsign_helpers as SS
from tests.test_precedence_cpu import _usage

ROOT = os.path.dirname(SS.HERE)
INF = SS.INF


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SS.build_ref(tmp_path_factory.mktemp('stopsign_ref'))


def both(ref, w, log=None):
    """one step through the host build (forwards and backwards) and the restatement on copies of w: the words after it, all three the same"""
    a, b, t = (SS.copy_words(w) for _ in range(3))
    n = [SS.host_rule(ref, a), SS.host_rule(ref, b, backwards=True), SS.rule_python(t, log=log)]
    assert len(set(n)) == 1 and n[0] == int(a['n_waiting'].sum()), n
    assert SS.same(a, b) == [] and SS.same(a, t) == [], (SS.same(a, b), SS.same(a, t))
    for k in w:         # nothing else is written
        if k not in SS.OUT_KEYS and isinstance(w[k], np.ndarray):
            assert a[k].tobytes() == w[k].tobytes(), k
    assert (a['cut_len'] <= w['cut_len']).all()
    return a


@pytest.mark.parametrize('n_per', SS.N_PER)
def test_rule_on_random_junctions(ref, n_per):
    """S1.  seeded random junctions at this n_per with 1, 12 and 16 movements, all-way and two-way, 64 / G + 1 junctions each, three
    consecutive steps so that stamps, stickiness and the clock carry over: host build = restatement, byte for byte (lag bitwise), walking
    the junctions forwards and backwards; cut_len is only lowered and nothing but the rule's words is written"""
    for seed, n, n_moves, J, signed in SS.case_set():
        if n != n_per:
            continue
        w = SS.random_words(seed, n_per, n_moves, J, signed)
        for step in range(SS.STEPS):
            after = both(ref, w)
            assert after['lag'].dtype == np.float64 and (after['clock'] != w['clock']).all()
            w = after
            SS.drive_on(w, seed, step)


def test_every_outcome_occurs(ref):
    """S2.  over the case set of S1, in the very steps in which the host build is compared with the restatement, every outcome occurs at
    least once: stamped in this step, released, denied by occ, by lane & ahead, by the blocked mask of an aged car in a junction and step in
    which a car crossing a denied car that is not aged is let through, by lag < gap; held by stickiness although it cannot stop, exempt,
    counted by ran, healed after done"""
    log = {}
    for seed, n_per, n_moves, J, signed in SS.case_set():
        w = SS.random_words(seed, n_per, n_moves, J, signed)
        for step in range(SS.STEPS):
            w = both(ref, w, log=log)
            SS.drive_on(w, seed, step)
    for k in SS.COUNTS:
        assert log.get(k, 0) > 0, (k, log)


def words_of(w, q):
    return (int(w['go'][q]), int(w['stopped_at'][q]), int(w['stopping'][q]), int(w['cut_len'][q]))


def test_crossing_arms_that_stamp_together(ref):
    """S3.  two cars on crossing arms stand in their zones in the same step: both stamp, the lower index goes first, the other is held at
    its line and goes only after the first has left the crossing"""
    w = SS.hand_words([(SS.A_, 18, 0.0), (SS.C_, 8, 0.0)], clock=5)
    w = both(ref, w)
    assert words_of(w, 0) == (1, 5, 0, 40) and words_of(w, 1) == (0, 5, 1, 10) and (w['occupied'][0], w['n_waiting'][0], w['clock'][0]) == (1, 1, 6)
    SS.move_to(w, [22, 8], [2.0, 0.0])      # the first is inside
    w = both(ref, w)
    assert words_of(w, 0)[0] == 1 and words_of(w, 1) == (0, 5, 1, 10) and w['occupied'][0] == 1
    SS.move_to(w, [30, 8])                  # at its exit: OUT
    w = both(ref, w)
    assert words_of(w, 0) == (0, -1, 0, 40) and words_of(w, 1) == (1, 5, 0, 10) and (w['occupied'][0], w['n_waiting'][0], w['ran'][0]) == (4, 0, 0)


def test_opposed_straights_go_together(ref):
    """S4.  movements 2 and 3 do not cross: two cars that stamp in the same step are released together"""
    w = both(ref, SS.hand_words([(SS.C_, 8, 0.0), (SS.D_, 13, 0.3)]))
    assert words_of(w, 0) == (1, 0, 0, 40) and words_of(w, 1) == (1, 0, 0, 40) and (w['occupied'][0], w['n_waiting'][0]) == (12, 0)


def test_a_car_behind_another_in_its_lane(ref):
    """S5.  movement 3 is inside; the car of movement 0 that stopped first crosses it and is denied; the car of movement 1 behind it in the
    same lane crosses nothing that is inside and is denied all the same (lane & ahead) -- and is released at once where the first car is
    not in front of it"""
    w = SS.hand_words([(SS.D_, 20, 3.0), (SS.A_, 18, 0.0), (SS.B_, 17, 0.0)], clock=9)
    w['stopped_at'][1], w['stopped_at'][2] = 4, 7
    w = both(ref, w)
    assert words_of(w, 1) == (0, 4, 1, 20) and words_of(w, 2) == (0, 7, 1, 20) and (w['occupied'][0], w['n_waiting'][0], w['ran'][0]) == (8, 2, 1)
    alone = SS.hand_words([(SS.D_, 20, 3.0), (SS.A_, 5, 0.0), (SS.B_, 17, 0.0)], clock=9)
    alone['stopped_at'][2] = 7
    alone = both(ref, alone)
    assert words_of(alone, 2) == (1, 7, 0, 40) and alone['occupied'][0] == 10


def test_two_way_stop_waits_for_a_gap(ref):
    """S6.  two-way: movements 2 and 3 are the through road.  A stopped car of movement 0 waits while the unsigned car's eta is below its
    gap of 3 s -- 4 m at 2 m/s --, with its lag and blocker written, and goes in the step in which it is not -- 4 m at 1 m/s; the unsigned
    car is never held and the car of movement 1, which movement 3 does not cross, has no lag"""
    w = SS.hand_words([(SS.A_, 18, 0.0), (SS.C_, 2, 2.0), (SS.B_, 12, 0.0)], sign=SS.TWO_WAY)
    w = both(ref, w)
    assert words_of(w, 0) == (0, 0, 1, 20) and (w['lag'][0], w['blocker'][0]) == (2.0, 1) and words_of(w, 1) == (0, -1, 0, 40)
    assert words_of(w, 2) == (0, -1, 1, 20) and (w['lag'][2], w['blocker'][2]) == (INF, -1)      # (outside its zone: no stamp yet, held)
    SS.move_to(w, v=[0.0, 1.0, 0.0])
    w = both(ref, w)
    assert words_of(w, 0) == (1, 0, 0, 20) and (w['lag'][0], w['blocker'][0]) == (4.0, 1) and words_of(w, 1) == (0, -1, 0, 40)
    assert (w['occupied'][0], w['n_waiting'][0]) == (1, 1)


def test_exemption_stickiness_and_ran(ref):
    """S7.  a car that comes into the detector too fast to stop is exempt and not held, and ran counts it once when it enters; one that was
    held in the step before stays held although it cannot stop any more"""
    w = SS.hand_words([(SS.A_, 15, 4.0), (SS.C_, 5, 4.0)])       # 2.5 m < 16 / 4
    w['stopping'][1] = 1
    w = both(ref, w)
    assert words_of(w, 0) == (0, -1, 0, 40) and words_of(w, 1) == (0, -1, 1, 10) and w['ran'][0] == 0
    SS.move_to(w, [20, 5])
    w = both(ref, w)
    assert words_of(w, 0)[0] == 1 and (w['ran'][0], w['occupied'][0]) == (1, 1)
    w = both(ref, w)
    assert w['ran'][0] == 1


def test_defective_words_are_data(ref):
    """S8.  a defective negative traj_idx, an index outside the tables, a line beyond the route's end: OUT, their words reset; a clock word
    at INT32_MAX stamps with it and wraps into the negative words, which count as 0"""
    w = SS.hand_words([(SS.A_, -2 ** 31, 0.0), ((168, 10), 5, 0.0), ((-9, 10), 5, 0.0), ((161, 9), 0, 0.0), (SS.C_, 8, 0.0), (SS.A_, -3, 0.0)],
                      clock=SS.INT32_MAX)
    w['go'][:4], w['stopped_at'][:4], w['stopping'][:4] = 1, 3, 1
    w = both(ref, w)
    for q in range(4):
        assert words_of(w, q)[:3] == (0, -1, 0) and (w['lag'][q], w['blocker'][q]) == (INF, -1)
    assert words_of(w, 4) == (1, SS.INT32_MAX, 0, 40) and w['clock'][0] == SS.INT32_MIN
    assert words_of(w, 5)[:3] == (0, -1, 0)     # (a line 23 points ahead: beyond the detector)
    w = both(ref, w)
    assert w['clock'][0] == 1 and words_of(w, 4)[0] == 1


def test_struct_mirror_matches_the_header(ref):
    """S9.  _lib.StopSignC against the layout the header's own compiler gives mpcx_stopsign and the field names parsed from the header;
    the junction limit agrees with _lib; the new exports are there; the structs it travels beside keep their sizes"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 36)()
    ref.stopsign_ref_layout(lay)
    names = [n for n, _ in _lib.StopSignC._fields_]
    assert names == ['path_stop', 'path_move', 'path_exit', 'conflict', 'lane', 'sign', 'gap', 'stopped_at', 'go', 'stopping', 'clock', 'ran', 'lag',
                     'blocker', 'occupied', 'n_waiting', 'v_stop', 'brake', 'v_floor', 'zone', 'detect', 'patience', 'n_per', 'n_junctions', 'n_moves',
                     'n_points', 'reserved']
    assert C.sizeof(_lib.StopSignC) == 184 == 16 * 8 + 3 * 8 + 8 * 4
    assert list(lay)[:28] == [C.sizeof(_lib.StopSignC)] + [getattr(_lib.StopSignC, n).offset for n in names]
    assert lay[28] == _lib.STOPSIGN_PER_MAX == 64
    assert list(lay)[29:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.PriorityC), C.sizeof(_lib.BrakingC),
                              C.sizeof(_lib.KeepClearC), C.sizeof(_lib.ReservationC), C.sizeof(_lib.SignalsC)]
    assert list(lay)[31:34] == [136, 40, 80]
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_stopsign;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_set_stopsign', 'mpcx_stopsign_step_batch'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_sign_table():
    """S10.  sign_table(): all-way by default, the named arms' three movements otherwise"""
    from mpc_for_av_at_intersection_amd.batch import sign_table
    assert sign_table().tolist() == [1] * 12 and sign_table().dtype == np.int32
    assert sign_table((1, 3)).tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert sign_table((0,), n_arms=2).tolist() == [1, 1, 1, 0, 0, 0]
    for bad in (dict(signed=(4,)), dict(n_arms=6), dict(n_arms=0)):
        with pytest.raises(ValueError):
            sign_table(**bad)


def test_stopsign_kernels_need_no_scratch():
    """S11.  mpcx_stopsign.hip cross-compiled for gfx950 with the Makefile's flags: exactly the seven lane-group instantiations of its one
    kernel (G = 1 .. 64), none with scratch, spills or LDS"""
    use = _usage('mpcx_stopsign.hip')
    assert len(use) == 7 and all('stopsign_kernel' in k for k in use), sorted(use)
    assert sorted(int(re.search(r'stopsign_kernelILi(\d+)E', k).group(1)) for k in use) == [1, 2, 4, 8, 16, 32, 64]
    for name, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (name, u)
