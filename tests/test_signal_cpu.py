"""Traffic signals (mpcx_signals) without a GPU: the host build of the rule (csrc/mpcx_signal_core.h through
tests/signal_ref/signal_ref.cpp; signal_kernel compiles the very same header) against a numpy restatement on hand-made words, the same
program under the sanitizers, the rule on the CPU oracle -- the four straight routes that gridlock under yield-to-everybody
(tests/test_precedence_cpu.py) clear under a two-phase plan with the phases never inside the crossing together --, the stop lines of the
stock routes, the ctypes mirror and the new file's kernel.  The device side is tests/test_gpu_signal.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import scene_helpers as SH
from tests import signal_helpers as G
from tests.test_precedence_cpu import _usage

ROOT = G.ROOT
# the straight scene under signal_helpers.PLAN (cycle 100, green 30, amber 8, all-red 12; T = 13, v0 = 0, cut mode, departure on), recorded
# from the CPU oracle: arms 1 and 3 go in the first green, arms 2 and 4 wait at their lines for 50 steps and go in the second
ARRIVALS = [56, 98, 56, 98]
WORST_CLEARANCE = 3.174182316982919


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return G.build_ref(tmp_path_factory.mktemp('signal_ref'))


def test_rule_on_hand_made_words(ref):
    """S1.  22 agents, two routes, two plans (signal_helpers.hand_made lists what each agent is there for).  The host build visiting the
    lanes forwards and backwards and the numpy restatement give identical cut_len, tick and held, byte for byte, and they are the values
    written down by hand: no line ahead, on and past the line, GREEN, AMBER (can stop, cannot stop, sticky) and RED, a retired agent,
    every defective entry, the tick's wrap at cycle - 1, a negative and an over-range tick, a conflict cut shorter than s."""
    w, want = G.hand_made()
    fwd, bwd, twin = G.copy_words(w), G.copy_words(w), G.copy_words(w)
    n = [G.host_rule(ref, fwd), G.host_rule(ref, bwd, backwards=True), G.rule_numpy(twin)]
    assert n == [int((want[:, 0] != 0).sum())] * 3 == [7] * 3
    for k in ('cut_len', 'tick', 'held'):
        assert fwd[k].tobytes() == bwd[k].tobytes() == twin[k].tobytes() and fwd[k].dtype == np.int32, k
    got = np.stack([fwd['held'], fwd['cut_len'], fwd['tick']], axis=1)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
    assert sorted(set(fwd['held'].tolist())) == [0, 1, 2]
    for k in w:         # nothing else is written
        if k not in ('cut_len', 'tick', 'held') and isinstance(w[k], np.ndarray):
            assert fwd[k].tobytes() == w[k].tobytes(), k
    # without the retirement words agent 9 is held like agent 4
    free = G.copy_words(w); free['done'] = None
    assert G.host_rule(ref, free) == 8 and (free['held'][9], free['cut_len'][9], free['tick'][9]) == (1, 20, 7)
    twin = G.copy_words(w); twin['done'] = None
    assert G.rule_numpy(twin) == 8 and all(twin[k].tobytes() == free[k].tobytes() for k in ('cut_len', 'tick', 'held'))


def test_host_build_under_sanitizers(ref, tmp_path):
    """S2.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on S1's
    words, forwards and backwards, with and without the retirement words, and on an empty case: no report, and the bytes of the plain build"""
    exe = str(tmp_path / 'signal_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DSIGNAL_REF_MAIN'] + G.INC + ['-o', exe, G.SRC], check=True)
    blob, want = b'', b''
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    for back in (0, 1):
        for with_done in (True, False):
            w, _ = G.hand_made()
            if not with_done:
                w['done'] = None
            blob += G.blob(w, back)
            got = G.host_rule(ref, w, backwards=bool(back))
            want += w['cut_len'].tobytes() + w['tick'].tobytes() + w['held'].tobytes() + i32(got)
    w, _ = G.hand_made()
    empty = G.words(**{k: (v[:0] if isinstance(v, np.ndarray) and k not in ('path_stop', 'path_group', 'plan_cycle', 'plan_amber', 'plan_green')
                           else v) for k, v in w.items()})
    blob += G.blob(empty, 0)
    want += i32(0)
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert open(outp, 'rb').read() == want and len(want) == 4 * (3 * 22 + 1) * 4 + 4


def test_straight_scene_clears_under_a_two_phase_plan():
    """S3.  Four straight stock routes from index 0 (T = 13, v0 = 0, cut mode, departure on) -- the scene tests/test_precedence_cpu.py shows
    gridlocking for 600 steps under yield-to-everybody -- under two_phase_plan(cycle 100, green 30, amber 8), which leaves 12 steps of
    all-red after each phase.  Every agent arrives within 600 steps; the true clearance between the present, driving agents stays positive
    at the start of every step; no two agents of different phases are inside the crossing square in the same step.  The arrival steps and
    the worst clearance are pinned as the oracle gives them.  Arms 2 and 4 wait at their lines through the first half cycle."""
    loop = G.straight_loop()
    hist = loop.run(600)
    held = [sum(1 for s in hist if s[a] is not None and s[a]['held']) for a in range(4)]
    print('arrivals', loop.arrival, 'worst clearance %r m' % loop.worst_clearance, 'held steps', held, 'mixed', loop.mixed_steps)
    assert all(loop.done) and max(loop.arrival) <= 600
    assert loop.worst_clearance > 0.0
    assert loop.mixed_steps == []
    assert loop.arrival == ARRIVALS and len(hist) == max(ARRIVALS)
    assert loop.worst_clearance == pytest.approx(WORST_CLEARANCE, abs=1e-9)
    assert held == [0, 50, 0, 50]
    # a held agent's path ends on the point before its line, and it waits there: it never passes index s while held
    s = int(loop.stop[1][0])
    for a in (1, 3):
        assert all(st[a]['cut'] == s and st[a]['traj_idx'] < s for st in hist[:50]) and hist[50][a]['held'] == 0


def test_all_green_is_the_run_without_signals():
    """S4.  With every group green for the whole cycle nobody is ever held: 20 steps equal the run without signals bit for bit"""
    paths, dl, start, stop, group = G.straight_scene()
    plan = dict(cycle=7, amber=0, green=np.array([[0, 7], [3, 7], [6, 7], [2, 7]]))
    a = G.SignalOracleLoop(paths, dl, start, stop, group, plan, tick=[0, 5, 9, -2], T=13, depart=True)
    b = SH.OracleLoop(paths, dl, start, T=13, depart=True)
    for s in range(20):
        ra, rb = a.step(), b.step()
        assert a.state.tobytes() == b.state.tobytes() and a.applied.tobytes() == b.applied.tobytes(), s
        assert all(ra[k]['cut'] == rb[k]['cut'] and ra[k]['held'] == 0 for k in range(4)), s
    assert a.prev == b.prev and a.traj_idx == b.traj_idx


def test_stop_lines_of_the_stock_routes():
    """S5.  stop_lines on the eight stock routes: every route has exactly one line, outside the crossing square, inside the route and at
    least the setback of arc before the square; both tables are consistent with each other and the group is the approach arm"""
    from mpc_for_av_at_intersection_amd.batch import stop_lines, two_phase_plan
    pairs = [(a, t) for a in (1, 2, 3, 4) for t in (1, 2)]
    routes = [H.smoothed_path(*pr) for pr in pairs]
    stop, group = stop_lines(routes)
    assert stop.dtype == group.dtype == np.int32 and len(stop) == len(group) == sum(len(r) for r in routes)
    off = 0
    for (arm, _), r in zip(pairs, routes):
        st, gr = stop[off:off + len(r)], group[off:off + len(r)]
        off += len(r)
        lines = sorted(set(st[st >= 0].tolist()))
        assert len(lines) == 1
        s = lines[0]
        assert 0 < s < len(r) - 1 and max(abs(r[s, 0]), abs(r[s, 1])) > 12.0
        assert (st[:s + 1] == s).all() and (st[s + 1:] == -1).all()
        assert (gr[:s + 1] == arm - 1).all() and (gr[s + 1:] == 0).all()
        first = int(np.flatnonzero(np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) <= 12.0)[0])
        arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(r[:, 0]), np.diff(r[:, 1])))])
        assert arc[first] - arc[s] >= 6.0 > arc[first] - arc[s + 1] and s < first
    # other setbacks move the line; a route that starts inside the square has none
    assert stop_lines(routes, setback=10.0)[0][0] < stop[0] < stop_lines(routes, setback=2.0)[0][0]
    assert (stop_lines([routes[0][300:]])[0] == -1).all() and (stop_lines(routes, setback=40.0)[0] == -1).all()
    assert len(stop_lines([])[0]) == 0
    pl = two_phase_plan(100, 30, 8)
    assert pl['cycle'] == 100 and pl['amber'] == 8 and pl['green'].tolist() == [[0, 30], [50, 30], [0, 30], [50, 30]]
    with pytest.raises(ValueError):
        two_phase_plan(100, 45, 8)


def test_struct_mirror_matches_the_header(ref):
    """S6.  _lib.SignalsC against the layout the header's own compiler gives mpcx_signals and the field names parsed from the header; the
    group limit agrees with _lib; the new exports are there; every older struct keeps its size"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 24)()
    ref.signal_ref_layout(lay)
    names = [n for n, _ in _lib.SignalsC._fields_]
    assert names == ['path_stop', 'path_group', 'plan_cycle', 'plan_amber', 'plan_green', 'plan_of', 'tick', 'held', 'brake', 'n_points', 'n_plans',
                     'n_groups', 'reserved']
    assert C.sizeof(_lib.SignalsC) == 88
    assert list(lay)[:14] == [C.sizeof(_lib.SignalsC)] + [getattr(_lib.SignalsC, n).offset for n in names]
    assert lay[14] == _lib.SIGNAL_GROUPS_MAX == 16
    assert list(lay)[15:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC),
                              C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC), C.sizeof(_lib.RespawnC), C.sizeof(_lib.RoutesC),
                              C.sizeof(_lib.PrecedenceC)]
    assert list(lay)[16:] == [24, 80, 32, 16, 40, 56, 64, 24]
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_signals;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_signals', 'mpcx_signal_step_batch'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_signal_kernel_needs_no_scratch():
    """S7.  mpcx_signal.hip cross-compiled for gfx950 with the Makefile's flags: exactly its one kernel, no scratch, no spills and no LDS"""
    use = _usage('mpcx_signal.hip')
    assert len(use) == 1 and 'signal_kernel' in next(iter(use)), sorted(use)
    u = next(iter(use.values()))
    assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, u
