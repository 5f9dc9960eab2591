"""The front end's kernels of csrc/mpcx_prepare.hip without a GPU: cross-compiled for gfx950 with the Makefile's flags, rollout_kernel and
ref_window_kernel (both RETIRE variants each) keep their names, need no scratch and spill nothing.  (predict_kernel: the same check in
tests/test_scene_cpu.py.)  The device side is tests/test_gpu_frontend_layout.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prepare_kernels_need_no_scratch():
    mk = open(os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('-I$(ROOT)/include', '-I' + os.path.join(ROOT, 'include'))
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (.*)$', mk, re.M).group(1).strip()
    src = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'mpcx_prepare.hip')
    assert os.path.exists(hipcc), 'no hipcc at %s (set HIPCC): the kernels cannot be cross-compiled for this check' % hipcc
    res = subprocess.run([hipcc] + flags.split() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-S', '-o', os.devnull, src],
                         check=True, capture_output=True, text=True)
    use, cur = {}, None
    for k, v in re.findall(r'remark:\s+([A-Za-z ]+(?: \[[^\]]*\])?): (\S+) \[-Rpass-analysis', res.stderr):
        if k == 'Function Name':
            cur = use.setdefault(v, {})
        elif cur is not None:
            cur[k.strip()] = int(v) if v.isdigit() else v
    roll = {n: u for n, u in use.items() if 'rollout_kernel' in n}
    win = {n: u for n, u in use.items() if 'ref_window_kernel' in n}
    print('rollout_kernel:', roll)
    print('ref_window_kernel:', win)
    # <false> and <true> of each: ...ILb0EE... / ...ILb1EE...
    for kernels in (roll, win):
        assert len(kernels) == 2 and sorted('ILb1E' in n for n in kernels) == [False, True], sorted(kernels)
    for n, u in list(roll.items()) + list(win.items()):
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0, (n, u)
