"""Reduced frames, host side: options.frames / options.frame_spec read from the YAML text beside the sanitised dictionaries and
checked on the host; the six entry points in the header, the library and _lib; the row of the series table; the refusals of
SlabProblem and Ensemble; and the order of a block mean (csrc/frames.hpp) restated in NumPy -- frame_mean, which
tests/test_gpu_frames.py holds the device against -- tested on its own.  No GPU."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('gpf_frames_set', 'gpf_frames_clear', 'gpf_frames_read', 'gpf_frames_now', 'gpf_frames_shape', 'gpf_frames_time')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def frame_mean(F, window, stride):
    """csrc/frames.hpp, restated: F (..., Nx, Ny) holds the terms of the interior cells (the stride-1 sample frame of the whole
    interior).  Block (a, b) of the window cut from its corner (ix0, iy0): per column a sum from +0.0 over the block's rows in
    ascending ix; those sums added from +0.0 in ascending iy; one division by (double)(rows * cols).  Returns (..., mx, my)."""
    ix0, ix1, iy0, iy1 = window
    sx, sy = stride
    mx, my = -(-(ix1 - ix0 + 1) // sx), -(-(iy1 - iy0 + 1) // sy)
    out = np.empty(F.shape[:-2] + (mx, my))
    for a in range(mx):
        r0 = ix0 + a * sx
        r1 = min(r0 + sx - 1, ix1)
        for b in range(my):
            c0 = iy0 + b * sy
            c1 = min(c0 + sy - 1, iy1)
            total = np.zeros(F.shape[:-2])
            for iy in range(c0, c1 + 1):
                column = np.zeros(F.shape[:-2])
                for ix in range(r0, r1 + 1):
                    column = column + F[..., ix - 1, iy - 1]
                total = total + column
            out[..., a, b] = total / np.float64((r1 - r0 + 1) * (c1 - c0 + 1))
    return out


def parsed(more, keep='_keep_frames'):
    from gapflow_amd import problem
    from gapflow_amd.io import read_yaml_input
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    getattr(problem, keep)(d, text)
    return d, before


@pytest.mark.parametrize('keep', ['_keep_frames', '_keep_own_options'])
def test_keys_are_read_from_the_yaml_text(keep):
    d, _ = parsed(", frames: 5", keep)
    assert d['options']['frames'] == 5 and 'frame_spec' not in d['options']
    d, _ = parsed(", frames: 0", keep)          # 0: off, like an absent key
    assert d['options']['frames'] == 0
    d, _ = parsed(", frames: 2, frame_spec: {fields: [p, rho, h], window: [2, 99, 1, 5], stride: [8, 2], reduce: mean, dtype: f8, capacity: 3}", keep)
    assert d['options']['frames'] == 2
    assert d['options']['frame_spec'] == {'fields': ['rho', 'p', 'h'], 'window': [2, 99, 1, 5], 'stride': [8, 2], 'reduce': 'mean', 'dtype': 'f8',
                                          'capacity': 3}
    d, _ = parsed(", frames: 1, frame_spec: {reduce: mean}", keep)       # the defaults; a mean over blocks of one cell is a sample
    assert d['options']['frame_spec'] == {'fields': ['rho', 'jx', 'jy', 'p'], 'window': None, 'stride': [1, 1], 'reduce': 'sample', 'dtype': 'f4',
                                          'capacity': None}


def test_absent_keys_leave_the_dictionaries_unchanged():
    for keep in ('_keep_frames', '_keep_own_options'):
        d, before = parsed("", keep)
        if keep == '_keep_own_options':
            assert d['options'].pop('checkpoint_freq') == 0         # (the one key that is always written)
        assert d == before and 'frames' not in d['options'] and 'frame_spec' not in d['options']


@pytest.mark.parametrize('bad', ["frames: -1", "frames: 1.5", "frames: True", "frames: [1]",
                                 "frame_spec: {fields: [rho, q]}", "frame_spec: {fields: []}", "frame_spec: {fields: [p, p]}", "frame_spec: {fields: p}",
                                 "frame_spec: {window: [0, 5, 1, 6]}", "frame_spec: {window: [1, 101, 1, 6]}", "frame_spec: {window: [1, 100, 1, 7]}",
                                 "frame_spec: {window: [9, 3, 1, 6]}", "frame_spec: {window: [1, 100, 4, 2]}", "frame_spec: {window: [1, 100, 1]}",
                                 "frame_spec: {window: [1, 100, 1, 2.5]}", "frame_spec: {stride: [0, 1]}", "frame_spec: {stride: [1, 65]}",
                                 "frame_spec: {stride: [2]}", "frame_spec: {stride: 2}", "frame_spec: {stride: [True, 1]}",
                                 "frame_spec: {reduce: max}", "frame_spec: {reduce: 1}", "frame_spec: {dtype: f2}", "frame_spec: {dtype: float32}",
                                 "frame_spec: {capacity: 0}", "frame_spec: {capacity: 1.5}", "frame_spec: {every: 2}", "frame_spec: [rho]"])
def test_bad_keys_raise(bad):
    with pytest.raises(ValueError, match=r'^(frames|options\.frame_spec): '):
        parsed(", " + bad)


def test_spec_is_checked_and_completed_on_the_host():
    from gapflow_amd.series import _frame_axes, _frame_shape, _frame_spec, _frame_window, _frames_stride
    assert _frames_stride(3) == 3 and _frames_stride(0, allow_zero=True) == 0
    for bad in (0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='frames: the stride must be an integer >= 1'):
            _frames_stride(bad)
    s = _frame_spec()
    assert s == {'fields': ('rho', 'jx', 'jy', 'p'), 'window': None, 'stride': [1, 1], 'reduce': 'sample', 'dtype': 'f4', 'capacity': None}
    assert _frame_window(s, 48, 37) == (1, 48, 1, 37) and _frame_shape(s, 48, 37) == (48, 37)
    # the record's order is the library's, whatever the order given
    assert _frame_spec({'fields': ('tau_yz_top', 'h', 'rho')})['fields'] == ('rho', 'h', 'tau_yz_top')
    # sx = sy = 1 is normalised to sample; any other stride keeps mean
    assert _frame_spec({'reduce': 'mean', 'stride': (1, 1)})['reduce'] == 'sample'
    assert _frame_spec({'reduce': 'mean', 'stride': (1, 2)})['reduce'] == 'mean' and _frame_spec({'reduce': 'mean', 'stride': (2, 1)})['reduce'] == 'mean'
    # without a grid only the order of the window is checked; with one, its extent
    assert _frame_spec({'window': (1, 500, 1, 500)})['window'] == [1, 500, 1, 500]
    with pytest.raises(ValueError, match='inside the interior'):
        _frame_spec({'window': (1, 500, 1, 500)}, 48, 37)
    # ragged blocks: 37 rows in blocks of 3 from row 5, 30 columns in blocks of 5 from column 4
    s = _frame_spec({'window': (5, 41, 4, 33), 'stride': (3, 5), 'reduce': 'mean'}, 48, 37)
    assert _frame_shape(s, 48, 37) == (13, 6)
    x, y = _frame_axes(s, 48, 37, 2.0, 10.0)
    # the mean of the block's cell centres (ix - 0.5) dx: rows 5..7 -> 5.5, the ragged last block is row 41 alone
    np.testing.assert_array_equal(x[:2], [2.0 * 5.5, 2.0 * 8.5])
    assert x[-1] == 2.0 * 40.5 and y[0] == 10.0 * 5.5 and y[-1] == 10.0 * 30.5 and x.shape == (13,) and y.shape == (6,)
    s = _frame_spec({'window': (5, 41, 4, 33), 'stride': (3, 5)}, 48, 37)          # sample: the first cell's
    x, y = _frame_axes(s, 48, 37, 2.0, 10.0)
    np.testing.assert_array_equal(x, 2.0 * (np.arange(5, 42, 3) - 0.5))
    np.testing.assert_array_equal(y, 10.0 * (np.arange(4, 34, 5) - 0.5))


def test_header_declares_the_entry_points_and_the_library_exports_them():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    text = open(os.path.join(ROOT, 'include', 'gapflow_hip.h')).read()
    assert 'gpf_frame_spec' in re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(build_library())
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), f'{name} is not declared in include/gapflow_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES['gpf_frames_time'] == _lib.SIGNATURES['gpf_lines_time']
    assert _lib.SIGNATURES['gpf_frames_clear'] == _lib.SIGNATURES['gpf_lines_clear']
    assert ctypes.sizeof(_lib.GpfFrameSpec) == 36 and [f[0] for f in _lib.GpfFrameSpec._fields_] == \
        ['fields', 'ix0', 'ix1', 'iy0', 'iy1', 'sx', 'sy', 'reduce', 'dtype']
    assert _lib.FRAME_FIELDS == _lib.LINE_FIELDS and _lib.FRAME_REDUCE == ('sample', 'mean') and _lib.FRAME_DTYPES == ('f8', 'f4')
    # a null handle is refused before anything is touched (no device needed)
    for name, args in (('gpf_frames_set', (None, 1, None, 0)), ('gpf_frames_clear', (None,)), ('gpf_frames_read', (None, None, 0, None, None)),
                       ('gpf_frames_now', (None, None, None, 0)), ('gpf_frames_shape', (None, None, None, None, None)),
                       ('gpf_frames_time', (None, 1, 0, None))):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        assert fn(*args) == -1, name


def test_the_row_sits_ahead_of_the_changes_row():
    import inspect
    from gapflow_amd import Problem
    from gapflow_amd.series import ALL_SERIES, CUTS, SERIES, SERIES_MORE
    assert ALL_SERIES == SERIES + SERIES_MORE
    assert [r.marker for r in SERIES_MORE] == ['_frames_every', '_changes_every']
    row = SERIES_MORE[0]
    assert (row.marker, row.recorder, row.collect, row.write) == ('_frames_every', '_frames_rec', '_collect_frames', '_write_frames')
    assert (row.noun, row.clear, row.fused) == ('frames', 'clear_frames', True)
    assert row.refusal[1] == CUTS == "they cut the batch per member"
    assert row.refusal[0] > max(r.refusal[0] for r in ALL_SERIES if r.refusal and r is not row)
    assert "self._frames_every" in inspect.getsource(Problem.__init__)
    for name in (row.collect, row.write, row.clear, 'set_frames', 'frame_now'):
        assert callable(getattr(Problem, name))
    assert isinstance(Problem.frames, property)
    sig = inspect.signature(Problem.set_frames)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != 'self'] == \
        [('every', 1), ('fields', ('rho', 'jx', 'jy', 'p')), ('window', None), ('stride', (1, 1)), ('reduce', 'sample'), ('dtype', 'f4'),
         ('capacity', None), ('keep', None)]


def member(frames_every, **armed):
    """What Ensemble's host-side refusal reads of a Problem, without a device behind it."""
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape, p.grid = (102, 3), {'Nx': 100, 'Ny': 1}
    p._integral_every, p._probe_cells, p._extrema_every, p._changes_every, p._frames_every = None, None, None, None, frames_every
    for k, v in armed.items():
        setattr(p, k, v)
    return p


def test_ensemble_names_the_armed_member_and_the_reason(monkeypatch):
    from gapflow_amd import Ensemble
    from gapflow_amd.ensemble import _refusal
    monkeypatch.delenv('GPF_SMALL_GRID', raising=False)
    assert _refusal(member(None)) is None
    assert _refusal(member(2)) == (NotImplementedError, "frames are armed on it (they cut the batch per member): clear_frames(), or run it alone")
    with pytest.raises(NotImplementedError, match=r'member 1: frames are armed on it .*clear_frames\(\)'):
        Ensemble([member(None), member(2)])
    # behind every other series in the order of the refusals
    assert _refusal(member(2, _changes_every=1))[1].startswith('changes are armed')
    assert _refusal(member(2, _extrema_every=1))[1].startswith('extrema are armed')
    text = open(os.path.join(ROOT, 'gapflow_amd', 'csrc', 'api_ensemble.inc')).read()
    assert 'frames are armed on it (they cut the batch per member; gpf_frames_clear, or step it alone)' in text


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='frames: not available on a SlabProblem'):
        SlabProblem.set_frames(object(), every=2)
    with pytest.raises(NotImplementedError, match='frames: not available on a SlabProblem'):
        SlabProblem.frame_now(object())


def test_restated_mean_on_exact_data_is_the_block_mean():
    """Small integers add exactly in any order: the restatement must give the exact block means, ragged ends, single-row and
    single-column blocks included, and leave every window cell in exactly one block."""
    rng = np.random.default_rng(7)
    F = rng.integers(-1000, 1000, size=(2, 11, 7)).astype(np.float64)
    for window in ((1, 11, 1, 7), (2, 10, 3, 7), (4, 4, 1, 7), (1, 11, 5, 5), (3, 3, 2, 2)):
        ix0, ix1, iy0, iy1 = window
        for stride in ((2, 2), (3, 5), (7, 3), (64, 64), (1, 4), (4, 1), (1, 1), (11, 7), (10, 6)):
            sx, sy = stride
            got = frame_mean(F, window, stride)
            mx, my = -(-(ix1 - ix0 + 1) // sx), -(-(iy1 - iy0 + 1) // sy)
            assert got.shape == (2, mx, my)
            cells = 0
            for a in range(mx):
                for b in range(my):
                    block = F[:, ix0 - 1 + a * sx:min(ix0 - 1 + (a + 1) * sx, ix1), iy0 - 1 + b * sy:min(iy0 - 1 + (b + 1) * sy, iy1)]
                    cells += block.shape[1] * block.shape[2]
                    np.testing.assert_array_equal(got[:, a, b], block.sum(axis=(1, 2)) / np.float64(block.shape[1] * block.shape[2]))
            assert cells == (ix1 - ix0 + 1) * (iy1 - iy0 + 1)
    # blocks of one cell: the cells themselves (the library stores such a frame as a sample and never adds)
    np.testing.assert_array_equal(frame_mean(F, (2, 10, 3, 7), (1, 1)), F[:, 1:10, 2:7])


def test_restated_mean_adds_rows_first_then_columns():
    """Data on which the order shows: with a = 1e16 a column (a, 1) sums to a (the 1 is lost) and a column (-a, 1) to -a, so rows
    first gives 0 for the block [[a, -a], [1, 1]]; columns first -- (a + -a) + (1 + 1) -- would give 2."""
    a = 1e16
    F = np.array([[a, -a], [1.0, 1.0]])
    assert frame_mean(F, (1, 2, 1, 2), (2, 2))[0, 0] == 0.0
    assert frame_mean(F.T.copy(), (1, 2, 1, 2), (2, 2))[0, 0] == 2.0 / 4.0      # transposed: the columns are (a, -a) and (1, 1)
    # every sum starts from +0.0: a block of -0.0 has the mean +0.0, where its sample keeps the sign
    Z = np.full((3, 3), -0.0)
    assert not np.signbit(frame_mean(Z, (1, 3, 1, 3), (3, 3))[0, 0]) and not np.signbit(frame_mean(Z, (1, 3, 1, 3), (1, 2))[0, 0])
    # single-row and single-column blocks add along the other axis alone, ascending
    R = np.array([[1.0, a, -a, 1.0]])
    assert frame_mean(R, (1, 1, 1, 4), (1, 4))[0, 0] == ((((0.0 + 1.0) + a) + -a) + 1.0) / 4.0
    assert frame_mean(R.T.copy(), (1, 4, 1, 1), (4, 1))[0, 0] == ((((0.0 + 1.0) + a) + -a) + 1.0) / 4.0
