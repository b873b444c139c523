"""CPU sanitizer build of the through-gap profile arithmetic (csrc/closures.hpp profile_coefficients / profile_at, the
functions k_gap_profiles runs): tests/hostcheck/profiles_host.cpp compiled with g++ -fsanitize=address,undefined must
reproduce tests/golden/leaf_profiles.npz (true outputs of the reference's models/profiles.py) to 1e-13 of each output's
scale, with no sanitizer report."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from profile_cases import cases, scale_close

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostcheck', 'profiles_host.cpp')
MODES = {'both': 0, 'top': 1, 'bottom': 2, 'none': 3}


@pytest.fixture(scope='module')
def profiles_host(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is part of the image'
    exe = str(tmp_path_factory.mktemp('hostcheck') / 'profiles_host')
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
           SRC, '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def case_stream(kind, kw, shape):
    """Header and arrays of one case, every input spelled out per cell (the program checks the arithmetic, the Python
    wrapper the broadcasting)."""
    nz, cells = shape[0], shape[1:]
    n = int(np.prod(cells, dtype=np.int64)) if cells else 1
    z = np.broadcast_to(kw['z'], shape).reshape(nz, n)
    per = lambda a: np.broadcast_to(np.asarray(a, float), cells).reshape(n)
    comp = lambda a: np.stack([per(np.asarray(a, float)[c]) for c in range(3)])
    stress = kind == 'stress'
    mode = MODES[kw['mode'] if stress else kw['slip']]
    zero = np.zeros((3, n))
    parts = [[mode, nz, n, 1.0 if stress else 0.0, kw['U'], kw['V']], z, comp(kw['q'])]
    if stress:
        parts += [comp(kw['h']), comp(kw['dqx']), comp(kw['dqy']), per(kw['eta']), per(kw['zeta'])]
    else:
        parts += [zero, zero, per(0.0), per(0.0)]
    parts.append(per(kw['Ls']))
    return [np.asarray(p, float).ravel() for p in parts], (8, nz) + tuple(cells)


def test_host_profiles_match_reference_outputs_under_sanitizers(profiles_host):
    all_cases = cases()
    stream, shapes = [np.array([float(len(all_cases))])], []
    for key, kind, kw, ref in all_cases:
        parts, oshape = case_stream(kind, kw, ref.shape[1:])
        stream += parts
        shapes.append(oshape)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([profiles_host], input=np.concatenate(stream).tobytes(), capture_output=True, env=env)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    assert res.stderr == b'', 'sanitizer output:\n' + res.stderr.decode()[-3000:]
    out = np.frombuffer(res.stdout, dtype=float)
    assert out.size == sum(int(np.prod(s)) for s in shapes)
    pos = 0
    for (key, kind, kw, ref), s in zip(all_cases, shapes):
        got = out[pos:pos + int(np.prod(s))].reshape(s)
        pos += got.size
        got = got[:2] if kind == 'velocity' else got[2:]
        for c in range(ref.shape[0]):
            scale_close(got[c], ref[c], 1e-13)
    assert len(all_cases) == 60
