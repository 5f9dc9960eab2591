"""Crossing reservations (mpcx_reservation) without a GPU: the host build of the rule (csrc/mpcx_reserve_core.h through
tests/reserve_ref/reserve_ref.cpp; reserve_kernel compiles the very same header) against a numpy restatement on hand-made junctions, the
same program under the sanitizers, the movement tables of the stock routes, the rule on the CPU oracle -- the straight scene, the four left
turns and the eight-agent scene all clear, and no two cars of conflicting movements are ever inside the crossing together --, the ctypes
mirror and the new file's kernels.  The device side is tests/test_gpu_reserve.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import reserve_helpers as RH
from tests.test_precedence_cpu import _usage

ROOT = RH.ROOT
SIZES = (1, 3, 8, 64)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return RH.build_ref(tmp_path_factory.mktemp('reserve_ref'))


@pytest.mark.parametrize('n_per', SIZES)
def test_rule_on_hand_made_junctions(ref, n_per):
    """R1.  reserve_helpers.CASES (and WIDE at n_per = 64), one junction per case with the expected words beside it, at n_per = 1, 3, 8
    and 64.  The host build walking the junctions forwards and backwards and the numpy restatement give identical grant, since, clock,
    occupied, queued, held and cut_len, byte for byte, and they are the values written down by hand; nothing else is written."""
    w, want = RH.hand_made(n_per)
    fwd, bwd, twin, twin_b = (RH.copy_words(w) for _ in range(4))
    n = [RH.host_rule(ref, fwd), RH.host_rule(ref, bwd, backwards=True), RH.rule_numpy(twin), RH.rule_numpy(twin_b, backwards=True)]
    assert len(set(n)) == 1 and n[0] == sum(1 for v in want[3].values() if v[2]), n
    for k in RH.OUT_KEYS:
        assert fwd[k].tobytes() == bwd[k].tobytes() == twin[k].tobytes() == twin_b[k].tobytes() and fwd[k].dtype == np.int32, k
    RH.check_against_want(fwd, want, w)
    J = len(w['mgr_of'])
    assert J == sum(1 for c in RH.CASES if len(c[3]) <= n_per) + (len(RH.WIDE) if n_per == 64 else 0) and (n_per < 3 or J >= len(RH.CASES)) and J >= 14
    if n_per >= 3:
        assert sorted(set(fwd['held'].tolist())) == [0, 1] and fwd['queued'].max() >= 2 and (fwd['grant'] != w['grant']).any()
    if n_per == 64:
        assert fwd['queued'][-3:].tolist() == [0, 63, 63] and fwd['grant'][-192:-128].all()
    for k in w:         # nothing else is written
        if k not in RH.OUT_KEYS and isinstance(w[k], np.ndarray):
            assert fwd[k].tobytes() == w[k].tobytes(), k
    # without the retirement words the done agent keeps its grant and the crossing: the car it had let in is denied
    if n_per >= 2:
        free = RH.copy_words(w); free['done'] = None
        twin = RH.copy_words(free)
        assert RH.host_rule(ref, free) == RH.rule_numpy(twin) == n[0] + 1
        assert all(free[k].tobytes() == twin[k].tobytes() for k in RH.OUT_KEYS)
        j = next(i for i, c in enumerate(c for c in RH.CASES if len(c[3]) <= n_per) if c[0].startswith('a done agent'))
        assert (free['occupied'][j], free['queued'][j]) == (1, 1) and (fwd['occupied'][j], fwd['queued'][j]) == (4, 0)


def test_host_build_under_sanitizers(ref, tmp_path):
    """R2.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on R1's
    junctions at every size, forwards and backwards, with and without the retirement words, and on an empty case: no report, and the bytes
    of the plain build"""
    exe = str(tmp_path / 'reserve_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DRESERVE_REF_MAIN'] + RH.INC + ['-o', exe, RH.SRC], check=True)
    blob, want = b'', b''
    for n_per in SIZES:
        for back in (0, 1):
            for with_done in (True, False):
                w, _ = RH.hand_made(n_per)
                if not with_done:
                    w['done'] = None
                blob += RH.blob(w, back)
                want += RH.out_bytes(w, RH.host_rule(ref, w, backwards=bool(back)))
    w, _ = RH.hand_made(3)
    empty = RH.words(**{k: (v[:0] if k in RH.PER_AGENT + RH.PER_JUNCTION else v) for k, v in w.items()})
    blob += RH.blob(empty, 0)
    want += np.array([0], np.int32).tobytes()
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert open(outp, 'rb').read() == want and len(want) > 4 * 4 * 7 * 17


def test_movement_tables_of_the_stock_routes():
    """R3.  movement_lines() and movement_conflicts() on the 12 stock routes (tests/helpers.smoothed_path(sp, ti), disc centres 2.18 / 0.68,
    radius sqrt 2): stop is stop_lines()', every line at index 144, the exits of the straight routes at 555, the movement index is
    3 (sp - 1) + (ti - 1), the conflict words are the 31 pairs computed for the issue at margins 0, 1 and 1.5, lane[g] = 7 << 3 (g / 3)."""
    from mpc_for_av_at_intersection_amd.batch import movement_conflicts, movement_lines, stop_lines
    pairs = [(sp, ti) for sp in (1, 2, 3, 4) for ti in (1, 2, 3)]
    routes = [H.smoothed_path(sp, ti) for sp, ti in pairs]
    stop, group, ex = movement_lines(routes)
    assert np.array_equal(stop, stop_lines(routes)[0]) and stop.dtype == group.dtype == ex.dtype == np.int32
    offs = np.cumsum([0] + [len(r) for r in routes])
    for k, (sp, ti) in enumerate(pairs):
        s, g, e = (t[offs[k]:offs[k + 1]] for t in (stop, group, ex))
        assert s[0] == 144 and (s[:145] == 144).all() and (s[145:] == -1).all(), (sp, ti)
        assert 144 < e[0] < len(routes[k]) and (e[:e[0]] == e[0]).all() and (e[e[0]:] == -1).all(), (sp, ti)
        assert (g[:e[0]] == 3 * (sp - 1) + (ti - 1)).all() and not g[e[0]:].any(), (sp, ti)
        if ti == 2:
            assert e[0] == 555
        r = routes[k]
        inside = np.flatnonzero(np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) <= 12.0)
        arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(r[:, 0]), np.diff(r[:, 1])))])
        assert arc[e[0]] - arc[inside[-1]] >= 4.0 > arc[e[0] - 1] - arc[inside[-1]]
    for margin in (0.0, 1.0, 1.5):
        conflict, lane = movement_conflicts(routes, stop, ex, [2.18, 0.68], np.sqrt(2.0), margin)
        assert conflict.tolist() == [1944, 3672, 592, 3523, 711, 640, 3614, 1593, 1033, 247, 459, 74], (margin, conflict.tolist())
        assert lane.tolist() == [7 << 3 * (g // 3) for g in range(12)] and conflict.dtype == lane.dtype == np.int32
        assert sum(bin(int(c)).count('1') for c in conflict) == 2 * 31
        assert all((int(conflict[g]) >> h) & 1 == (int(conflict[h]) >> g) & 1 for g in range(12) for h in range(12))
        assert not any(int(conflict[g]) & int(lane[g]) for g in range(12))
    # the (x, y) form of the disc offsets, as the interaction parameters hold them, gives the same words
    both = movement_conflicts(routes, stop, ex, [[2.18, 0.0], [0.68, 0.0]], np.sqrt(2.0))
    assert np.array_equal(both[0], conflict) and np.array_equal(both[1], lane)


@pytest.fixture(scope='module')
def oracle_runs():
    """the six oracle runs of R4, computed once: three scenes x patience 0 / unbounded"""
    runs = {}
    for name in ('straight', 'turn1', 'eight'):
        for patience in (0, None):
            loop = RH.scene_loop(name, patience)
            runs[name, patience] = (loop, loop.run(600))
    return runs


@pytest.mark.parametrize('name', ['straight', 'turn1', 'eight'])
@pytest.mark.parametrize('patience', [0, None], ids=['fcfs', 'first-fit'])
def test_scenes_clear_under_reservations(oracle_runs, name, patience):
    """R4.  The straight scene, the four (arm, 1) routes and the eight-agent scene of the precedence tests on a ReserveOracleLoop (T = 13,
    v0 = 0, cut mode, departure on, detector = the whole approach) with patience 0 and unbounded.  Everybody arrives within 600 steps; in
    no step are two cars of conflicting movements inside the crossing square together; the worst clearance is positive; every grant is
    given in a step whose occ before it holds no conflicting movement; in the first-fit straight run arms 1 and 3 are never held."""
    loop, hist = oracle_runs[name, patience]
    held = [sum(1 for s in hist if s[a] is not None and s[a]['held']) for a in range(loop.A)]
    print('reservations, %s, patience %s: arrivals %s, worst clearance %.2f m, held steps %s, grants %d, max queued %d'
          % (name, patience, loop.arrival, loop.worst_clearance, held, len(loop.grants), max(loop.queued_hist)))
    assert all(loop.done) and 0 < max(loop.arrival) <= 600
    assert loop.mixed_steps == []
    assert loop.worst_clearance > 0.0
    conflict = loop.tab['conflict']
    assert len(loop.grants) == loop.A and sorted(q for _, q, _, _ in loop.grants) == list(range(loop.A))
    for step, q, g, occ in loop.grants:
        assert int(conflict[g]) & occ == 0 and g == loop.movement[q], (step, q, g, occ)
    assert max(held) > 0 and max(loop.queued_hist) > 0
    if name == 'straight' and patience is None:
        assert held[0] == 0 and held[2] == 0 and held[1] > 0 and held[3] > 0


def test_struct_mirror_matches_the_header(ref):
    """R5.  _lib.ReservationC against the layout the header's own compiler gives mpcx_reservation and the field names parsed from the
    header; the junction limit agrees with _lib; the new exports are there; every older struct keeps its size"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 29)()
    ref.reserve_ref_layout(lay)
    names = [n for n, _ in _lib.ReservationC._fields_]
    assert names == ['path_exit', 'conflict', 'lane', 'mgr_time', 'mgr_of', 'grant', 'since', 'clock', 'occupied', 'queued', 'n_per', 'n_junctions',
                     'n_mgr', 'reserved']
    assert C.sizeof(_lib.ReservationC) == 96
    assert list(lay)[:15] == [C.sizeof(_lib.ReservationC)] + [getattr(_lib.ReservationC, n).offset for n in names]
    assert lay[15] == _lib.RESERVE_PER_MAX == 64
    assert list(lay)[16:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC),
                              C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC), C.sizeof(_lib.RespawnC), C.sizeof(_lib.RoutesC),
                              C.sizeof(_lib.PrecedenceC), C.sizeof(_lib.SignalsC), C.sizeof(_lib.ActuationC), C.sizeof(_lib.AdviceC),
                              C.sizeof(_lib.IntentC)]
    assert list(lay)[17:] == [24, 80, 32, 16, 40, 56, 64, 24, 88, 80, 40, 24]
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_reservation;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_reserved', 'mpcx_reserve_step_batch'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_reserve_kernels_need_no_scratch():
    """R5.  mpcx_reserve.hip cross-compiled for gfx950 with the Makefile's flags: exactly the seven lane-group instantiations of its one
    kernel (G = 1 .. 64), none with scratch, spills or LDS"""
    use = _usage('mpcx_reserve.hip')
    assert len(use) == 7 and all('reserve_kernel' in k for k in use), sorted(use)
    assert sorted(int(re.search(r'reserve_kernelILi(\d+)E', k).group(1)) for k in use) == [1, 2, 4, 8, 16, 32, 64]
    for name, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (name, u)
