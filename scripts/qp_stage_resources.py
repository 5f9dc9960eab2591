"""Static resources of the twelve instantiations of the stage-structured QP kernel (csrc/mpcx_qp_quad.hip): the numbers of DESIGN 4.1's
tables, taken from the compiler instead of counted by hand.

    python scripts/qp_stage_resources.py [--markdown] [--keep-asm FILE]

It compiles the file for the device only,

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/mpcx_qp_quad.hip

and prints per kernel: instructions between the kernel's label and its .Lfunc_end, how many of them are FP64, v_cndmask_b32, v_accvgpr_*,
v_readlane_b32, v_writelane_b32 (the last two move spilled scalar registers in and out of a VGPR), s_nop, s_waitcnt; and from the
resource remarks VGPR / AGPR / SGPR, spilled SGPRs and VGPRs, and scratch bytes per lane.  A tool, not a test: needs hipcc, no GPU."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'mpc_for_av_at_intersection_amd', 'csrc', 'mpcx_qp_quad.hip')
KERNEL = re.compile(r'^_ZN4mpcx14qp_quad_kernelILi8ELi(\d)ELb([01])ELb([01])EEEvNS_6QpArgsE$')
COUNTED = (('fp64', lambda m: '_f64' in m), ('cndmask', lambda m: m == 'v_cndmask_b32'), ('accvgpr', lambda m: m.startswith('v_accvgpr_')),
           ('readlane', lambda m: m == 'v_readlane_b32'), ('writelane', lambda m: m == 'v_writelane_b32'), ('s_nop', lambda m: m == 's_nop'),
           ('s_waitcnt', lambda m: m == 's_waitcnt'))
REMARKS = (('vgpr', 'VGPRs'), ('agpr', 'AGPRs'), ('sgpr', 'TotalSGPRs'), ('sgpr_spill', 'SGPRs Spill'), ('vgpr_spill', 'VGPRs Spill'),
           ('scratch', 'ScratchSize [bytes/lane]'))
COLUMNS = ('insts',) + tuple(k for k, _ in COUNTED) + tuple(k for k, _ in REMARKS)


def compile_asm(hipcc, asm_path):
    cmd = [hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + os.path.join(ROOT, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', SRC, '-o', asm_path]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit('hipcc failed')
    return r.stderr


def kernel_key(name):
    m = KERNEL.match(name)
    return None if m is None else (int(m.group(1)), m.group(3) == '1', m.group(2) == '1')      # (SPL, JERK, TUNED)


def parse_asm(text):
    out, cur = {}, None
    for line in text.splitlines():
        if cur is None:
            if not line[:1].isspace() and line.split(':', 1)[0] != line:
                key = kernel_key(line.split(':', 1)[0])
                if key is not None:
                    cur = out[key] = dict.fromkeys(('insts',) + tuple(k for k, _ in COUNTED), 0)
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        body = line.split(';', 1)[0].strip()
        if not body or body.startswith('.') or body.endswith(':'):
            continue
        mnem = body.split()[0]
        mnem = re.sub(r'_(e32|e64|dpp|sdwa|e64_dpp)$', '', mnem)
        cur['insts'] += 1
        for k, pred in COUNTED:
            cur[k] += bool(pred(mnem))
    return out


def parse_remarks(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark:\s+(.*?)\s*\[-Rpass-analysis', line)
        if m is None:
            continue
        what = m.group(1)
        if what.startswith('Function Name:'):
            key = kernel_key(what.split(':', 1)[1].strip())
            cur = None if key is None else out.setdefault(key, {})
        elif cur is not None:
            for k, label in REMARKS:
                if what.startswith(label + ':'):
                    cur[k] = int(what.split(':', 1)[1])
    return out


def name_of(key):
    spl, jerk, tuned = key
    return '<8,%d,%s,%s>' % (spl, 'true' if tuned else 'false', 'true' if jerk else 'false')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hipcc', default=os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))
    ap.add_argument('--markdown', action='store_true', help='print a markdown table')
    ap.add_argument('--keep-asm', metavar='FILE', help='keep the assembly text there')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm_path = args.keep_asm or os.path.join(tmp, 'mpcx_qp_quad.s')
        remarks = parse_remarks(compile_asm(args.hipcc, asm_path))
        with open(asm_path) as f:
            counts = parse_asm(f.read())
    if len(counts) != 12 or sorted(counts) != sorted(remarks):
        raise SystemExit('expected the twelve instantiations of qp_quad_kernel, found %d in the text and %d in the remarks' % (len(counts), len(remarks)))
    rows = [(name_of(k),) + tuple({**counts[k], **remarks[k]}[c] for c in COLUMNS) for k in sorted(counts)]
    head = ('kernel <LQ,SPL,TUNED,JERK>',) + COLUMNS
    if args.markdown:
        print('| ' + ' | '.join(head) + ' |')
        print('|' + '---|' * len(head))
        for r in rows:
            print('| ' + ' | '.join(str(v) for v in r) + ' |')
    else:
        fmt = '%-26s' + ' %10s' * len(COLUMNS)
        print(fmt % head)
        for r in rows:
            print(fmt % r)


if __name__ == '__main__':
    main()
