"""The contraction rule of k_wfilm_partial (csrc/weighted_kernels.hip): the accumulate acc += w * term rounds the product on its
own.  No run can see it from the ones and box planes -- fma(1.0, t, acc) is acc + t, fma(0.0, t, acc) is acc -- and the smooth
planes sit a thousand times inside their tolerance, so the ISA is what pins it.  The library is compiled with -ffp-contract=fast,
under which a contraction pragma alone does not hold the backend back; this compiles the Dowson-Higginson instantiations to gfx950
assembly with the library's flags, next to a copy of the file whose accumulate is the bare `a.v[k] += w * t[k]`, and counts: the
loop body has two cells of nine integrands, so the kernel must hold 18 fewer v_fma_f64, 18 more v_mul_f64 and 18 more v_add_f64
than the fused copy."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gapflow_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
ACCUMULATE = re.compile(r'#pragma clang fp contract\(off\)\n(\s*)a\.v\[k\] \+= __builtin_canonicalize\(w \* t\[k\]\);')


def counts(tmp, kernels_file, tag):
    """kernel name -> (v_fma_f64, v_mul_f64, v_add_f64, all instructions) of k_wfilm_partial<DH, false / true>"""
    src, asm = os.path.join(tmp, tag + '.hip'), os.path.join(tmp, tag + '.s')
    with open(src, 'w') as f:
        f.write('#include <hip/hip_runtime.h>\n#include "step_kernel.hip"\n#include "integral_kernels.hip"\n'
                f'#include "{kernels_file}"\n')
        for ls in ('false', 'true'):
            f.write(f'template __global__ void gpf::k_wfilm_partial<0, {ls}>(const gpf::WFilmArgs, const gpf::Phys, long long);\n')
    from gapflow_amd.build import FLAGS
    flags = [x for x in FLAGS if x not in ('-shared', '-fPIC')]
    subprocess.run([HIPCC] + flags + ['-I', CSRC, '-S', '--cuda-device-only', src, '-o', asm], check=True, capture_output=True, timeout=900)
    lines = open(asm).read().split('\n')
    out = {}
    for s in [i for i, l in enumerate(lines) if re.match(r'^_ZN3gpf15k_wfilm_partialI.*:', l)]:
        end = next(i for i in range(s, len(lines)) if lines[i].strip().startswith('.Lfunc_end'))
        body = [l.split(';')[0].strip() for l in lines[s + 1:end]]
        ops = [l.split()[0] for l in body if l and not l.startswith('.') and not l.endswith(':')]
        out[lines[s].split(':')[0]] = (sum(o.startswith(('v_fma_f64', 'v_fmac_f64')) for o in ops), sum(o.startswith('v_mul_f64') for o in ops),
                                        sum(o.startswith('v_add_f64') for o in ops), len(ops))
    assert len(out) == 2, sorted(out)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_weighted_accumulate_is_a_multiply_and_an_add():
    with open(os.path.join(CSRC, 'weighted_kernels.hip')) as f:
        text = f.read()
    fused_text, n = ACCUMULATE.subn(r'\1a.v[k] += w * t[k];', text)
    assert n == 1, "the accumulate statement of wfilm_cell is not where this test looks for it"
    with tempfile.TemporaryDirectory() as tmp:
        fused_file = os.path.join(tmp, 'weighted_fused.hip')
        with open(fused_file, 'w') as f:
            f.write(fused_text)
        kept = counts(tmp, os.path.join(CSRC, 'weighted_kernels.hip'), 'kept')
        fused = counts(tmp, fused_file, 'fused')
    for name in kept:
        (fma, mul, add, total), (fma0, mul0, add0, total0) = kept[name], fused[name]
        print(f"\n{name}: v_fma_f64 {fma} (fused copy {fma0}), v_mul_f64 {mul} ({mul0}), v_add_f64 {add} ({add0}), instructions {total} ({total0})")
        assert (fma0 - fma, mul - mul0, add - add0) == (18, 18, 18), (name, kept[name], fused[name])
