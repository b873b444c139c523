"""Host side of checkpoint and restart: the file format, the atomic write, the command line and the ctypes table (no GPU)."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest


def test_file_header_round_trips(tmp_path):
    from gapflow_amd import checkpoint
    meta = {'kind': 'problem', 'inputs': checkpoint.input_dicts({'output': 'x', 'silent': True}, {'Nx': np.int64(7), 'dx': np.float64(0.1) / 3,
                                                                                                'bc_xE_P': (True, True, False)},
                                                                {'tol': 1e-300, 'max_it': 10**12}, {'EOS': 'DH', 'elastic': {'E': 5e10}}, {'U': -0.0}),
            'mirror': {'residual_buffer': deque([1.0, 2.5e-7], 5), 'history': {'step': [0, 25], 'ekin': [np.float64(1) / 3, 2.0]}}}
    blob = bytes(range(256)) * 3
    path = str(tmp_path / 'c.gpf')
    checkpoint.write_file(path, meta, blob)
    got, got_blob = checkpoint.read_file(path)
    assert bytes(got_blob) == blob
    assert got['inputs']['grid'] == {'Nx': 7, 'dx': 0.1 / 3, 'bc_xE_P': [True, True, False]}
    assert got['inputs']['numerics'] == {'tol': 1e-300, 'max_it': 10**12}
    assert got['inputs']['properties']['elastic']['E'] == 5e10
    assert np.signbit(got['inputs']['geometry']['U'])
    assert got['mirror']['residual_buffer'] == [1.0, 2.5e-7] and got['mirror']['history']['ekin'][0] == 1 / 3
    assert tuple(got['inputs']) == checkpoint.INPUT_KEYS
    assert not os.path.exists(path + '.tmp')


def test_damaged_files_are_refused(tmp_path):
    from gapflow_amd import checkpoint
    data = checkpoint.pack({'kind': 'problem'}, b'12345678' * 10)
    assert checkpoint.unpack(data)[0] == {'kind': 'problem'}
    with pytest.raises(ValueError, match='truncated'):
        checkpoint.unpack(data[:-1])
    with pytest.raises(ValueError, match='truncated'):
        checkpoint.unpack(data[:10])
    with pytest.raises(ValueError, match='magic'):
        checkpoint.unpack(b'X' + data[1:])
    with pytest.raises(ValueError, match='version'):
        checkpoint.unpack(data[:8] + b'\x07\x00\x00\x00' + data[12:])


def test_atomic_write_keeps_the_old_file(tmp_path, monkeypatch):
    from gapflow_amd import checkpoint
    path = str(tmp_path / 'c.gpf')
    checkpoint.write_file(path, {'n': 1}, b'old state')
    before = open(path, 'rb').read()

    def interrupted(src, dst):
        raise OSError("interrupted")
    monkeypatch.setattr(os, 'replace', interrupted)
    with pytest.raises(OSError, match='interrupted'):
        checkpoint.write_file(path, {'n': 2}, b'new state, longer than the old one')
    assert open(path, 'rb').read() == before
    assert checkpoint.read_file(path) == ({'n': 1}, b'old state')


def test_restart_argument_parses():
    from gapflow_amd.__main__ import make_parser, restart_overrides
    cli = make_parser()
    o = cli.parse_args(['--restart', 'out/checkpoint.gpf'])
    assert o.restart == 'out/checkpoint.gpf' and o.filename is None and restart_overrides(o) == (None, None)
    o = cli.parse_args(['--restart', 'c.gpf', '--output', 'again', '--max-it', '500', '--device', '2'])
    assert restart_overrides(o) == ({'output': 'again'}, {'max_it': 500}) and o.device == 2
    o = cli.parse_args(['-i', 'input.yaml'])
    assert o.filename == 'input.yaml' and o.restart is None
    for bad in ([], ['-i', 'a.yaml', '--restart', 'c.gpf']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_ctypes_signatures_exist():
    from gapflow_amd import _lib
    s = _lib.SIGNATURES
    assert s['gpf_checkpoint_size'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)])
    assert s['gpf_checkpoint_save'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)])
    assert s['gpf_checkpoint_load'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t])
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'gapflow_hip.h')).read()
    for name in ('gpf_checkpoint_size', 'gpf_checkpoint_save', 'gpf_checkpoint_load'):
        assert f'int {name}(' in header


def test_checkpoint_freq_is_kept_beside_the_sanitised_options():
    """The sanitiser's output is pinned to the reference's keys; the key of this project rides beside it (default 0 = off)."""
    import contextlib
    import io
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_checkpoint_freq
    for text, want in (("options: {output: x, checkpoint_freq: 10}\n", 10), ("options: {output: x}\n", 0)):
        with contextlib.redirect_stdout(io.StringIO()):
            d = read_yaml_input(io.StringIO(text))
        assert 'checkpoint_freq' not in d['options']
        _keep_checkpoint_freq(d, text)
        assert d['options']['checkpoint_freq'] == want
