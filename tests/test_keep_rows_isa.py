"""The keep-set of k_step2 (csrc/step2_kernel.hip): with non-temporal stores, the rows with (ix & 7) < k are stored plain so that
they stay in the Infinity Cache for the next step, every other row `nt`.  Both forms live in one inline-asm statement; hipcc has
merged a hinted and a plain store before and dropped the hint.  This compiles the x-only-gap Dowson-Higginson instantiations the
benchmark runs (both march directions) and the 2-D-gap one to gfx950 assembly and checks that every march store of a 16-byte pair
has both forms, each its own instruction, side by side."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gapflow_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
VARIANTS = ['0, false, false, 1, 3', '0, false, false, -1, 3', '0, false, false, 1, 0']


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_march_stores_carry_the_nt_and_the_keep_form():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, 't.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include "step_kernel.hip"\n#include "aux_kernels.hip"\n#include "step2_kernel.hip"\n'
                    'using namespace gpf;\n')
            for v in VARIANTS:
                f.write(f'template __global__ void gpf::k_step2<{v}>(const Step2Args, const Phys);\n')
        asm = os.path.join(tmp, 't.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=fast', '-I', CSRC, '-S', '--cuda-device-only',
                        src, '-o', asm], check=True, capture_output=True, timeout=900)
        lines = open(asm).read().split('\n')
    starts = [i for i, l in enumerate(lines) if re.match(r'^_ZN3gpf7k_step2I.*:', l)]
    assert len(starts) == len(VARIANTS)
    for s in starts:
        end = next(i for i in range(s, len(lines)) if lines[i].strip().startswith('.Lfunc_end'))
        body = [l.strip() for l in lines[s:end]]
        stores = [l for l in body if l.startswith('global_store_dwordx4')]
        forms = {}
        for l in stores:
            pol = l.split(' off', 1)[1].strip() if ' off' in l else 'saddr'
            forms[pol] = forms.get(pol, 0) + 1
        name = lines[s].split(':')[0]
        # three planes per row, one statement each, holding both forms (plain 16-byte stores outside the march exist too)
        assert forms.get('nt', 0) >= 3 and forms.get('', 0) >= forms.get('nt'), (name, forms)
        assert not any(k.startswith('sc') for k in forms), (name, forms)
        # every `nt` store sits in an asm statement right behind its plain sibling
        for i, l in enumerate(body):
            if l.startswith('global_store_dwordx4') and l.endswith('off nt'):
                window = body[max(0, i - 4):i]
                assert any(w.startswith('global_store_dwordx4') and w.endswith(' off') for w in window), (name, body[i - 4:i + 1])
