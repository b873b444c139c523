"""Static instruction mix of k_step2's march loop, from the gfx950 assembly hipcc produces (CPU, cross-compile):

    python tools/step_isa_count.py [--csrc DIR] [--out FILE.json] ['EOS, HAS_LS, PIEZO, D, TOPO' ...]

For each named instantiation (default: the benchmarked x-only-gap kernel with the row coefficients evaluated in the kernel,
TOPO 3, and read from the table, TOPO 4 -- where the sources have it) the march loop is located -- the innermost loop that holds
the hand-written row loads -- and its instructions are counted by class: fp64 VALU, other VALU, SALU, SMEM (scalar loads), VMEM
(vector loads and stores), LDS, waits.  The loop body holds one copy of the row per row buffer (the buffers rotate by name), so the
figures are also given per ROW.  A row-load or store statement holds a plain and a non-temporal form behind a scalar branch; only
the form before the branch is counted, as one of the two executes.  Every block of the loop is counted, the ones a given wave or
row skips included (edge lanes' 8-byte stores, the ghost-column work of one strip, a chunk's first and last row): the figures
compare builds, they are not a trace.  Instruction classes only -- no timing model.
--csrc points at another checkout's gapflow_amd/csrc (the parent commit's, to compare)."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ['0, false, false, 1, 3', '0, false, false, 1, 4']


def executed_lines(body):
    """The loop's instruction lines; inside an inline-asm statement the alternative behind `s_branch` is left out."""
    out, in_asm, skipping = [], False, False
    for l in body:
        t = l.strip()
        if t.startswith(';;#ASMSTART'):
            in_asm, skipping = True, False
        elif t.startswith(';;#ASMEND'):
            in_asm, skipping = False, False
        elif not t or t[0] == ';' or (t[0] == '.' and not t.endswith(':')):
            continue
        elif t.endswith(':'):
            if in_asm and 'done' in t:
                skipping = False
        elif not skipping:
            out.append(t)
            if in_asm and t.startswith('s_branch'):
                skipping = True
    return out


def classify(ins):
    c = {'valu_fp64': 0, 'valu_other': 0, 'salu': 0, 'smem': 0, 'vmem': 0, 'lds': 0, 'wait_nop': 0, 'other': 0}
    for t in ins:
        op = t.split()[0]
        if op.startswith(('s_waitcnt', 's_nop')):
            c['wait_nop'] += 1
        elif op.startswith(('s_load', 's_buffer_load')):
            c['smem'] += 1
        elif op.startswith('s_'):
            c['salu'] += 1
        elif op.startswith('v_'):
            c['valu_fp64' if '_f64' in op else 'valu_other'] += 1
        elif op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
            c['vmem'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
        else:
            c['other'] += 1
    return c


def march_loop(fn):
    """(start, end, rows) of the inner loop that holds the hand-written row loads (the one with the most of them)."""
    best = None
    for h, l in enumerate(fn):
        m = re.match(r'^\.(LBB\d+_\d+):.*Inner Loop Header', l)
        if not m:
            continue
        name = m.group(1)[1:]
        end = max([i for i, x in enumerate(fn) if re.search(r'in Loop: Header=' + name + r'\b', x)] + [h])
        while end + 1 < len(fn) and not fn[end + 1].startswith(('.LBB', '; %bb.')):      # to the end of the loop's last block
            end += 1
        rows, in_asm, seen = 0, False, False
        for x in fn[h:end + 1]:
            t = x.strip()
            if t.startswith(';;#ASMSTART'):
                in_asm, seen = True, False
            elif t.startswith(';;#ASMEND'):
                in_asm = False
            elif in_asm and t.startswith('global_load_dwordx4') and not seen:
                rows, seen = rows + 1, True
        if rows and (best is None or rows > best[2]):
            best = (h, end, rows)
    return best


def main():
    args = sys.argv[1:]
    csrc, out = os.path.join(ROOT, 'gapflow_amd', 'csrc'), None
    if '--csrc' in args:
        i = args.index('--csrc'); csrc = os.path.abspath(args[i + 1]); del args[i:i + 2]
    if '--out' in args:
        i = args.index('--out'); out = args[i + 1]; del args[i:i + 2]
    has_table = 'TOPO == 4' in open(os.path.join(csrc, 'step2_kernel.hip')).read()
    variants = args or [v for v in DEFAULT if has_table or not v.endswith('4')]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, 't.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include "step_kernel.hip"\n#include "aux_kernels.hip"\n#include "step2_kernel.hip"\nusing namespace gpf;\n')
            for v in variants:
                f.write(f'template __global__ void gpf::k_step2<{v}>(const Step2Args, const Phys);\n')
        asm = os.path.join(tmp, 't.s')
        subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=fast', '-I', csrc, '-S',
                        '--cuda-device-only', src, '-o', asm], check=True, capture_output=True)
        text = open(asm).read().split('\n')
    result = {}
    starts = [i for i, l in enumerate(text) if re.match(r'^_ZN3gpf7k_step2I.*:', l)]
    for v, a in zip(variants, starts):
        b = next(i for i in range(a, len(text)) if text[i].startswith('.Lfunc_end'))
        fn = text[a:b]
        h, e, rows = march_loop(fn)
        c = classify(executed_lines(fn[h:e + 1]))
        c['valu'] = c['valu_fp64'] + c['valu_other']
        entry = {'symbol': text[a].split(':')[0], 'rows_per_loop_iteration': rows, 'per_loop_iteration': c,
                 'per_row': {k: round(n / rows, 2) for k, n in c.items()}}
        result[f'k_step2<{v}>'] = entry
        print(f'k_step2<{v}>', json.dumps(entry['per_row']), f'({rows} rows per iteration)')
    if out:
        json.dump(result, open(out, 'w'), indent=1, sort_keys=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
