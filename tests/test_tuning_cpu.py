"""The QP away from the stock parameters, on the CPU: the oracle and the one-lane host build of the stage solver (csrc/mpcx_qp_stage.h)
with a different parameter set per problem (tests/tuning_helpers.mixed: the sweep lattice of test_sensitivity_sweep_as_one_batch on the
warm-started problems of helpers.horizon_problems) against the exact minimiser of the literal problem (tests/qp_literal.py).  This is
the reference side of tests/test_gpu_tuning.py: where these pass and a HIP kernel misses the same bars on the same inputs, the fault is
in the device build (lane mapping, the row fetch, per-problem constants, the refill), not in the iteration."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import test_stage_ref as SR
from tests import tuning_helpers as TH

CASES = [(T, False) for T in (10, 13, 16, 20, 24, 32)] + [(T, True) for T in (13, 20, 28)]
IDS = ['%s%d' % ('jerk-' if j else 'T', T) for T, j in CASES]


@pytest.fixture(scope='module')
def stage_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('stage_ref') / 'libstage_ref.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wall', '-Wno-unknown-pragmas'] + SR.INC + ['-o', so, SR.SRC], check=True)
    return C.CDLL(so)


def test_parameter_sets_are_the_sweep_lattice():
    """16 sets, drawn as test_sensitivity_sweep_as_one_batch draws its first 16: all different, every one away from the stock parameters in
    several fields, and every tuned field takes at least two values across them (a field a kernel dropped would show)"""
    sets = TH.parameter_sets()
    rows = np.stack([TH.runtime_params(13, **s).tuning_row() for s in sets])
    assert rows.shape == (16, 16) and len({r.tobytes() for r in rows}) == 16
    stock = TH.runtime_params(13).tuning_row()
    assert ((rows != stock).sum(1) >= 3).all()
    varies = [len(set(rows[:, c].tolist())) > 1 for c in range(16)]
    assert varies == [True] * 8 + [False, True, False, True] + [True] * 3 + [False]      # Qf[0], Qf[2] and the padding word are fixed in the lattice
    first = rows[0]
    assert (first[0], first[1], first[12], first[13]) == (sets[0]['w_perp'], sets[0]['w_para'], sets[0]['max_accel'], sets[0]['max_decel'])


@pytest.mark.parametrize('T,jerk', CASES, ids=IDS)
def test_oracle_and_host_build_with_a_set_per_problem(stage_lib, T, jerk):
    """24 problems, problem i under set i % 16.  Oracle: status 0 everywhere, within 5e-6 (max) / 1e-7 (median) of the exact minimiser,
    which is a KKT point to rounding.  Host build of the stage solver (four-state model), the problem's own mpcx_mpc_params per call:
    status 0, iteration count within one of the oracle's, u and x within 1e-8 of it (tests/test_stage_ref.py's bar).  At least 20 of the
    24 problems take an iteration.  Measured: oracle - exact max 1.1e-8 / 2.0e-9 / 2.0e-9 / 2.6e-8 / 5.5e-9 / 1.6e-8 at T = 10 / 13 / 16 /
    20 / 24 / 32 and 4.5e-10 / 1.4e-8 / 1.5e-8 for the five-state model at 13 / 20 / 28 (medians 1e-11 .. 2e-10); host build - oracle at
    most 1.2e-10; 22 to 24 problems with iterations."""
    m, ref = TH.mixed(T, jerk), TH.reference(T, jerk)
    assert (ref.status == 0).all(), ref.status
    for ex in ref.exact:
        TH.check_exact(ex)
    n_con = int((ref.iters > 0).sum())
    print('%s T=%d: %d of 24 with iterations, |oracle - exact| max %.2e median %.2e' % ('five-state' if jerk else 'four-state', T, n_con, ref.dist.max(),
                                                                                        np.median(ref.dist)))
    assert ref.dist.max() < 5e-6 and np.median(ref.dist) < 1e-7, (ref.dist.max(), np.median(ref.dist))
    assert n_con >= 20, n_con
    if jerk:
        return
    vp = C.c_void_p
    worst = 0.0
    for k, (x0, xref, xbar, re, uw) in enumerate(m.probs):
        cp = m.params[k].to_c()
        a = [np.ascontiguousarray(v, np.float64) for v in (x0, xref, xbar, uw)]
        re8 = np.ascontiguousarray(re, np.uint8)
        x = np.zeros((4, T + 1)); u = np.zeros((2, T)); kkt = np.zeros(4); st = C.c_int32(-1); it = C.c_int32(-1)
        stage_lib.stage_ref_solve(C.byref(cp), a[0].ctypes.data_as(vp), a[1].ctypes.data_as(vp), a[2].ctypes.data_as(vp), re8.ctypes.data_as(vp),
                                  a[3].ctypes.data_as(vp), x.ctypes.data_as(vp), u.ctypes.data_as(vp), C.byref(st), C.byref(it), kkt.ctypes.data_as(vp))
        assert st.value == 0 and abs(it.value - ref.iters[k]) <= 1, (k, st.value, it.value, ref.iters[k])
        worst = max(worst, float(np.abs(u - ref.sol[k].u).max()), float(np.abs(x - ref.sol[k].x).max()))
    print('T=%d: |host build - oracle| %.2e' % (T, worst))
    assert worst < 1e-8, worst


def test_closed_loop_scene_has_conflicts_and_constrained_solves():
    """the scene of test_gpu_tuning.py's coupled closed loop (2 x 8 agents, T = 20, one set per agent, 6 steps) on the CPU oracle: every solve
    succeeds, some agent has a conflict and some solve is constrained -- the seed was chosen for that here"""
    out = TH.oracle_loop(TH.loop_scene())
    hit, iters, status = out[..., 0], out[..., 1], out[..., 2]
    print('closed loop on the oracle: %d agent-steps, %d with a conflict, %d constrained' % (hit.size, (hit >= 0).sum(), (iters > 0).sum()))
    assert (status == 0).all()
    assert (hit >= 0).any() and (hit == -1).any() and (iters > 0).any()
