"""Right of way (mpcx_precedence) without a GPU: the host build of the entry-order stamp (csrc/mpcx_precedence_core.h through
tests/precedence_ref/precedence_ref.cpp; precedence_stamp_kernel compiles the very same header) against a numpy restatement on hand-made
words, the same program under the sanitizers, the rule itself on the CPU oracle -- three scenes that gridlock or nearly so when everybody
yields to everybody and clear under the standing rule, with the arrival steps pinned --, the ctypes mirror and the new file's kernel.  The
device side is tests/test_gpu_precedence.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import precedence_helpers as PH

ROOT = PH.ROOT
# arrival steps under the standing rule, precedence = agent index, T = 13, v0 = 0, cut mode, departure on (established on the CPU oracle)
ARRIVALS = {'straight': [56, 66, 78, 93], 'turn1': [55, 93, 84, 80], 'eight': [48, 88, 113, 70, 135, 114, 120, 125]}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return PH.build_ref(tmp_path_factory.mktemp('precedence_ref'))


def test_stamp_on_hand_made_words(ref):
    """P1.  Eight agents in two windows of a 12-row pool (precedence_helpers.hand_made).  The host build visiting the lanes forwards and
    backwards and the numpy restatement give identical words, byte for byte.  Waiting agents (entered_step -1 and -5), the agent whose own
    row lies outside the pool and the rows of nobody keep their words; two agents that entered in the same step are ordered by window
    offset; an earlier entry is a smaller word whatever the offsets; the largest step whose word fits is not negative."""
    h = PH.hand_made()
    before = h['prec'].copy()
    fwd, bwd, twin = before.copy(), before.copy(), before.copy()
    args = (h['entered'], h['own'], h['off'], h['n_rows'])
    assert PH.host_stamp(ref, fwd, *args) == 5 and PH.host_stamp(ref, bwd, *args, backwards=True) == 5
    PH.stamp_numpy(twin, *args)
    assert fwd.tobytes() == bwd.tobytes() == twin.tobytes() and fwd.dtype == np.int32
    written = [0, 2, 3, 7, 9]
    untouched = [r for r in range(12) if r not in written]
    assert np.array_equal(fwd[untouched], before[untouched]) and not (fwd[written] == before[written]).any()
    assert fwd[[0, 2, 3, 7]].tolist() == [0, 7 * 64 + 2, 7 * 64 + 3, 3 * 64 + 1]
    assert fwd[2] < fwd[3] and fwd[7] < fwd[2] and fwd[0] < fwd[7]
    assert fwd[9] == ((2 ** 31 - 64) // 64) * 64 + 3 > 0
    again = fwd.copy()
    assert PH.host_stamp(ref, again, *args) == 5 and again.tobytes() == fwd.tobytes()        # the word of an agent in the scene does not move


def test_host_build_under_sanitizers(ref, tmp_path):
    """P2.  the same source with -fsanitize=address,undefined as a stand-alone program (its own main; never loaded into Python) on P1's
    words, forwards and backwards, and on an empty case: no report, and the bytes of the plain build"""
    exe = str(tmp_path / 'precedence_ref_asan')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-DPRECEDENCE_REF_MAIN'] + PH.INC + ['-o', exe, PH.SRC], check=True)
    blob, want = b'', b''
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    for back in (0, 1):
        h = PH.hand_made()
        blob += i32(len(h['entered']), h['n_rows'], back) + h['off'].tobytes() + h['own'].tobytes() + h['entered'].tobytes() + h['prec'].tobytes()
        got = PH.host_stamp(ref, h['prec'], h['entered'], h['own'], h['off'], h['n_rows'], backwards=bool(back))
        want += h['prec'].tobytes() + i32(got)
    blob += i32(0, 0, 0)
    want += i32(0)
    inp, outp = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    open(inp, 'wb').write(blob)
    res = subprocess.run([exe, inp, outp], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert open(outp, 'rb').read() == want and len(want) == 2 * 13 * 4 + 4


@pytest.mark.parametrize('name', ['straight', 'turn1', 'eight'])
def test_scene_clears_under_the_standing_rule(name):
    """P3.  The scene on the CPU oracle (T = 13, v0 = 0, cut mode, departure on, precedence = agent index): under the standing rule every
    agent arrives, at the pinned step, and the true clearance between the present, driving agents -- taken at the start of every step --
    stays positive throughout."""
    loop = PH.scene_loop(name)
    hist = loop.run(600)
    print(name, loop.arrival, 'worst clearance %.3f m' % loop.worst_clearance, 'in %d steps' % len(hist))
    assert loop.arrival == ARRIVALS[name] and len(hist) == max(ARRIVALS[name])
    assert loop.worst_clearance > 0.0


@pytest.mark.parametrize('name', ['straight', 'eight'])
def test_scene_gridlocks_when_everybody_yields(name):
    """P3.  The gap this closes: under the reference's yield-to-everybody nobody arrives within 600 steps in the straight and the
    eight-agent scenes -- at the end every car stands"""
    loop = PH.scene_loop(name, mode='all')
    hist = loop.run(600)
    print(name, 'yield to everybody: speeds after 600 steps', loop.state[:, 2])
    assert len(hist) == 600 and not any(loop.done) and loop.arrival == [-1] * loop.A
    assert np.abs(loop.state[:, 2]).max() < 0.05


def test_equal_words_are_the_mutual_yield():
    """P3.  All words equal: nobody yields to anybody in the rule's sense, and the run is the yield-to-everybody run bit for bit (20 steps of
    the straight scene)."""
    a, b = PH.scene_loop('straight', mode='all'), PH.scene_loop('straight')
    b.prec = [5] * 4
    for s in range(20):
        a.step(); b.step()
        assert a.state.tobytes() == b.state.tobytes() and a.applied.tobytes() == b.applied.tobytes(), s


def test_standing_row_reproduces_its_pose():
    """P3.  The defining property's footing: the reference's rollout (moving_obstacles_prediction.py:21-28, restated) of a standing row
    (x, y, 0, yaw, 0, 0) holds the pose in every frame, bit for bit"""
    row = PH.standing(np.array([[3.25, -7.125, 4.0, 0.7, 1.5, 0.2]]), [0])[0]
    assert row.tolist() == [3.25, -7.125, 0.0, 0.7, 0.0, 0.0]
    x, y, v, yaw, a, steer = row
    for _ in range(30):
        x, y = x + v * np.cos(yaw) * 0.2, y + v * np.sin(yaw) * 0.2
        v = v + a * 0.2
        yaw = yaw + v / 2.86 * np.tan(steer) * 0.2
        assert (x, y, v, yaw) == (3.25, -7.125, 0.0, 0.7)


def test_struct_mirror_matches_the_header(ref):
    """P4.  _lib.PrecedenceC against the layout the header's own compiler gives mpcx_precedence and the field names parsed from the header;
    the mode values, the window and the last step agree with _lib; the new exports are there; every older struct keeps its size"""
    from mpc_for_av_at_intersection_amd import _lib
    lay = (C.c_int64 * 17)()
    ref.precedence_ref_layout(lay)
    names = [n for n, _ in _lib.PrecedenceC._fields_]
    assert C.sizeof(_lib.PrecedenceC) == 24 and names == ['prec', 'stand', 'n_rows', 'mode']
    assert list(lay)[:5] == [C.sizeof(_lib.PrecedenceC)] + [getattr(_lib.PrecedenceC, n).offset for n in names]
    assert list(lay)[5:9] == [_lib.PRECEDENCE_FIXED, _lib.PRECEDENCE_ENTRY, _lib.PRECEDENCE_WINDOW, _lib.PRECEDENCE_MAX_STEP]
    assert _lib.PRECEDENCE_MAX_STEP * 64 + 63 <= 2 ** 31 - 1 < (_lib.PRECEDENCE_MAX_STEP + 1) * 64 + 63 and PH.WINDOW == _lib.PRECEDENCE_WINDOW
    assert list(lay)[9:] == [C.sizeof(_lib.ClosedLoopC), C.sizeof(_lib.ClosedLoopOptsC), C.sizeof(_lib.RunLogC), C.sizeof(_lib.RetireC),
                             C.sizeof(_lib.SceneC), C.sizeof(_lib.AdmitC), C.sizeof(_lib.RespawnC), C.sizeof(_lib.RoutesC)]
    assert list(lay)[10:] == [24, 80, 32, 16, 40, 56, 64]
    hdr = open(os.path.join(ROOT, 'include', 'mpcx.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} mpcx_precedence;', hdr).group(1), flags=re.S)
    assert re.findall(r'\*?\b([a-z_0-9]+)\b\s*(?=[,;])', body) == names
    for name in ('mpcx_closed_loop_run_precedence', 'mpcx_admit_step_batch_precedence'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def _usage(name):
    """kernel -> resource usage of csrc/<name> cross-compiled for gfx950 with the Makefile's flags"""
    mk = open(os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('-I$(ROOT)/include', PH.INC[0])
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (.*)$', mk, re.M).group(1).strip()
    assert os.path.exists(hipcc), 'no hipcc at %s (set HIPCC): the kernels cannot be cross-compiled for this check' % hipcc
    src = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', name)
    res = subprocess.run([hipcc] + flags.split() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-S', '-o', os.devnull, src],
                         check=True, capture_output=True, text=True)
    use, cur = {}, None
    for k, v in re.findall(r'remark:\s+([A-Za-z ]+(?: \[[^\]]*\])?): (\S+) \[-Rpass-analysis', res.stderr):
        if k == 'Function Name':
            cur = use.setdefault(v, {})
        elif cur is not None:
            cur[k.strip()] = int(v) if v.isdigit() else v
    print(name, use)
    return use


def test_stamp_kernel_needs_no_scratch():
    """P5.  mpcx_precedence.hip cross-compiled for gfx950 with the Makefile's flags: exactly its one kernel, no scratch, no spills and no
    LDS"""
    use = _usage('mpcx_precedence.hip')
    assert len(use) == 1 and 'precedence_stamp_kernel' in next(iter(use)), sorted(use)
    u = next(iter(use.values()))
    assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, u


def test_right_of_way_instantiations():
    """P5.  mpcx_interaction_prec.hip holds exactly the three right-of-way instantiations -- predict_kernel<false / true, true, true> and
    interaction_kernel<true, true, true> -- of the templates in mpcx_interaction_parts.h, none with scratch, spills or static LDS; the
    conflict search keeps five wavefronts per SIMD within 96 VGPRs"""
    use = _usage('mpcx_interaction_prec.hip')
    want = ('predict_kernelILb0ELb1ELb1EEE', 'predict_kernelILb1ELb1ELb1EEE', 'interaction_kernelILb1ELb1ELb1EEE')
    assert len(use) == 3 and all(sum(w in n for n in use) == 1 for w in want), sorted(use)
    for n, u in use.items():
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0 and u['LDS Size [bytes/block]'] == 0, (n, u)
        if 'interaction_kernel' in n:
            assert u['VGPRs'] <= 96 and u['Occupancy [waves/SIMD]'] == 5, u
