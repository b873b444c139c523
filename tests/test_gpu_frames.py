"""Reduced frames (gpf_frames_*, Problem.set_frames / frames / frame_now, options.frames): for each selected field of the lines' nine
one (mx, my) array over a window of the interior, sampled at the first cell of every sx x sy block or averaged over the block, as
float or double, recorded on the device while gpf_step advances whole batches.

Yardsticks.  The stride-1 sample frame of the whole interior equals, in every bit, the state (rho, jx, jy), the gap (h) and the
single-index lines of film_lines stacked over the rows (all nine: p and the stresses are the lines' bits, which
tests/test_gpu_lines.py holds against the probes and the oracle).  Every other sample frame is a NumPy slice of that one.  A mean
frame equals, in every bit, the order csrc/frames.hpp states, restated in NumPy (tests/test_frames_host.py: frame_mean) over that
stride-1 frame.  An f4 frame is astype(float32) of the f8 one.  Independently, the nine fields restated on the downloaded state
-- the state and the gap themselves, the stresses with oracle/closures.py as tests/test_gpu_lines.py: oracle_stresses has them, p
with models.pressure.eos_pressure, the host function tests/test_gpu_probes.py holds a probe's p to -- and averaged with np.mean
agree with the mean frame at rtol 1e-12 + atol 1e-13 max|field|, the per-cell tolerance tests/test_gpu_lines.py holds the stresses
to (p: rtol 1e-12 alone per cell in test_gpu_probes.py; the blocks' pressures here share a sign): a mean is a convex combination
of its cells, so their bound carries over, and the rounding of the at most 21 additions of a block here (<= 21 * 2^-53
max|field|) is far inside the absolute term.
Everything else is held bit for bit: a record is a pure function of the state, and recording only reads.

Grids: 48 x 37 asperity (odd Ny, ragged blocks); 24 x 300 (a window wider than one workgroup's run at sy = 3); the 1-D journal
100 x 1 (k_small_steps, where the batch is cut at the recorded steps); 16 x 40 with a slip-length field (the HAS_LS
instantiations); the 1-D power-law slider (a second equation of state)."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest

import test_gpu_integrals as ti
import test_gpu_probes as tp
from test_frames_host import frame_mean
from test_gpu_lines import ASPERITY, oracle_stresses
from test_gpu_probes import INCLINED_PL, JOURNAL_1D, SURROGATE, THINNING, quiet
from test_gpu_weighted import ELASTIC

pytestmark = pytest.mark.gpu

FIELDS = ('rho', 'jx', 'jy', 'p', 'h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')
GRID_48 = ASPERITY.replace('Nx: 45, Ny: 37', 'Nx: 48, Ny: 37')
TEXT = {'48x37': GRID_48, '24x300': ti.PIEZO_WIDE, '100x1': JOURNAL_1D, 'power-law': INCLINED_PL}
STRIDES = ((2, 2), (3, 5), (7, 3), (64, 64), (1, 4), (4, 1))
WINDOWS = {'48x37': (None, (5, 41, 4, 33)), '24x300': (None, (2, 23, 7, 291))}
NSTEPS = 3


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    view = np.uint32 if a.dtype == np.float32 else np.uint64
    same = a.view(view) == b.view(view)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ"


def build(name):
    return ti.build('slip-field') if name == 'slip-field' else tp.build(TEXT[name])


@functools.lru_cache(maxsize=None)
def state(name):
    """A problem advanced NSTEPS steps and the stride-1 f8 sample frame of its whole interior, (9, Nx, Ny); computed once per grid
    and only read by the tests."""
    p = build(name)
    p._advance(NSTEPS, honor_stop=False)
    f = p.frame_now(fields=FIELDS, dtype='f8')
    return p, np.stack([f[k] for k in FIELDS])


def window_of(p, window):
    return (1, p.grid['Nx'], 1, p.grid['Ny']) if window is None else window


@pytest.mark.parametrize('name', ['48x37', '24x300', '100x1', 'slip-field', 'power-law'])
def test_sample_of_the_whole_interior_is_the_state_the_gap_and_the_lines(hiplib, name):
    p, F = state(name)
    nx, ny = p.grid['Nx'], p.grid['Ny']
    f = p.frame_now(fields=FIELDS, dtype='f8')
    assert f['fields'] == FIELDS and f['window'] == (1, nx, 1, ny) and f['stride'] == (1, 1) and f['reduce'] == 'sample'
    assert all(f[k].dtype == np.float64 and f[k].shape == (nx, ny) for k in FIELDS) and np.all(np.isfinite(F))
    np.testing.assert_array_equal(f['x'], (np.arange(1, nx + 1) - 0.5) * p.grid['dx'])
    np.testing.assert_array_equal(f['y'], (np.arange(1, ny + 1) - 0.5) * p.grid['dy'])
    q = np.array(p.q)
    for c, k in enumerate(('rho', 'jx', 'jy')):
        same_bits(f[k], q[c, 1:-1, 1:-1], f'{name}: {k} against q')
    same_bits(f['h'], np.array(p.topo.full[0])[1:-1, 1:-1], f'{name}: h against the gap')
    # all nine: the single-index lines along y, one per row, eight per call
    for first in range(1, nx + 1, 8):
        rows = list(range(first, min(first + 8, nx + 1)))
        got = p.film_lines(lines=[{'along': 'y', 'at': i, 'name': f'r{i}'} for i in rows])
        for i in rows:
            for k in FIELDS:
                same_bits(f[k][i - 1], got[f'r{i}'][k], f'{name}: row {i}: {k} against film_lines')
    # mean at stride (1, 1) is stored as sample: the same bits, -0.0 included
    m = p.frame_now(fields=FIELDS, dtype='f8', reduce='mean')
    assert m['reduce'] == 'sample'
    for k in FIELDS:
        same_bits(m[k], f[k], f'{name}: mean at (1, 1): {k}')
    # a subset keeps the library's order and the bits
    sub = p.frame_now(fields=('tau_yz_top', 'p'), dtype='f8')
    assert sub['fields'] == ('p', 'tau_yz_top') and sorted(k for k in sub if k in FIELDS) == ['p', 'tau_yz_top']
    same_bits(sub['p'], f['p'], 'subset: p')
    same_bits(sub['tau_yz_top'], f['tau_yz_top'], 'subset: tau_yz_top')
    h_only = p.frame_now(fields=('h', 'rho'), dtype='f8')         # h without a stress: the gap's plane 0 alone is read
    same_bits(h_only['h'], f['h'], 'h without a stress')


@pytest.mark.parametrize('name', ['48x37', '24x300'])
def test_strided_sample_is_a_slice_of_the_full_frame(hiplib, name):
    p, F = state(name)
    for window in WINDOWS[name]:
        ix0, ix1, iy0, iy1 = window_of(p, window)
        for sx, sy in ((3, 5),) + (STRIDES if window is not None else ((64, 64), (1, 4))):
            f = p.frame_now(fields=FIELDS, window=window, stride=(sx, sy), dtype='f8')
            assert f['window'] == (ix0, ix1, iy0, iy1) and f['stride'] == (sx, sy)
            for c, k in enumerate(FIELDS):
                same_bits(f[k], F[c, ix0 - 1:ix1:sx, iy0 - 1:iy1:sy], f'{name}: window {window} stride {(sx, sy)}: {k}')
            np.testing.assert_array_equal(f['x'], (np.arange(ix0, ix1 + 1, sx) - 0.5) * p.grid['dx'])


@pytest.mark.parametrize('name', ['48x37', '24x300', 'slip-field', 'power-law'])
def test_mean_equals_the_restated_order(hiplib, name):
    p, F = state(name)
    for window in WINDOWS.get(name, (None,)):
        w = window_of(p, window)
        for stride in STRIDES:
            f = p.frame_now(fields=FIELDS, window=window, stride=stride, reduce='mean', dtype='f8')
            assert f['reduce'] == 'mean' and f['stride'] == stride
            want = frame_mean(F, w, stride)
            for c, k in enumerate(FIELDS):
                same_bits(f[k], want[c], f'{name}: window {window} stride {stride}: {k}')
    # the rho / jx / jy / p instantiation (no gap plane is read) gives the same bits as the nine-field one
    f = p.frame_now(stride=(3, 5), reduce='mean', dtype='f8')
    want = frame_mean(F[:4], window_of(p, None), (3, 5))
    for c, k in enumerate(FIELDS[:4]):
        same_bits(f[k], want[c], f'{name}: default fields: {k}')
    g = p.frame_now(fields=('h', 'jy'), stride=(3, 5), reduce='mean', dtype='f8')
    same_bits(g['h'], frame_mean(F[4], window_of(p, None), (3, 5)), f'{name}: h without a stress')
    same_bits(g['jy'], want[2], f'{name}: jy beside h')


def test_more_than_one_workgroup_along_y(hiplib):
    """24 x 300 at sy = 3: 85 blocks per workgroup, so the 100 blocks of the whole width take two; the block means around the seam
    (b = 84, 85) are those of the restated order, and the mean's x / y are the means of the blocks' cell centres."""
    p, F = state('24x300')
    f = p.frame_now(fields=FIELDS, stride=(7, 3), reduce='mean', dtype='f8')
    assert f['rho'].shape == (4, 100)
    want = frame_mean(F, (1, 24, 1, 300), (7, 3))
    for c, k in enumerate(FIELDS):
        same_bits(f[k][:, 80:90], want[c][:, 80:90], f'seam of the workgroups: {k}')
    np.testing.assert_allclose(f['y'], (np.arange(100) * 3 + 2 - 0.5) * p.grid['dy'], rtol=1e-15)
    np.testing.assert_allclose(f['x'], np.array([4.0, 11.0, 18.0, 23.0]) * p.grid['dx'] - 0.5 * p.grid['dx'], rtol=1e-15)


@pytest.mark.parametrize('name', ['48x37', '24x300', 'slip-field'])
def test_f4_is_the_f8_record_converted_once(hiplib, name):
    p, _ = state(name)
    for spec in ({'reduce': 'sample', 'stride': (1, 1)}, {'reduce': 'sample', 'stride': (3, 5), 'window': (2, 15, 4, 33)},
                 {'reduce': 'mean', 'stride': (3, 5)}, {'reduce': 'mean', 'stride': (7, 3), 'window': (2, 15, 4, 33)}):
        a = p.frame_now(fields=FIELDS, dtype='f8', **spec)
        b = p.frame_now(fields=FIELDS, dtype='f4', **spec)
        for k in FIELDS:
            assert b[k].dtype == np.float32
            same_bits(b[k], a[k].astype(np.float32), f'{name}: {spec}: {k}')
    assert p.frame_now(fields=('rho',))['rho'].dtype == np.float32          # the default


@pytest.mark.parametrize('name', ['48x37', 'slip-field'])
def test_mean_agrees_with_the_oracle(hiplib, name):
    from gapflow_amd.models.pressure import eos_pressure
    p, _ = state(name)
    q = np.array(p.q)
    ref = [q[0], q[1], q[2], np.broadcast_to(eos_pressure(q[0], p.prop), q[0].shape), np.array(p.topo.full[0])] + oracle_stresses(p, q)
    nx, ny = p.grid['Nx'], p.grid['Ny']
    worst = 0.0
    for (sx, sy), window in (((3, 5), None), ((7, 3), (2, 15, 4, 33))):
        ix0, ix1, iy0, iy1 = window_of(p, window)
        f = p.frame_now(fields=FIELDS, window=window, stride=(sx, sy), reduce='mean', dtype='f8')
        for k, r in zip(FIELDS, ref):
            r = np.asarray(r, dtype=np.float64)
            want = np.array([[np.mean(r[a:min(a + sx, ix1 + 1), b:min(b + sy, iy1 + 1)]) for b in range(iy0, iy1 + 1, sy)] for a in range(ix0, ix1 + 1, sx)])
            scale = np.abs(r[1:-1, 1:-1]).max()
            tol = 1e-12 * np.abs(want) + 1e-13 * scale
            err = np.abs(f[k] - want)
            worst = max(worst, (err[tol > 0] / tol[tol > 0]).max(initial=0.0))
            np.testing.assert_allclose(f[k], want, rtol=1e-12, atol=1e-13 * scale, err_msg=f'{name}: stride {(sx, sy)} window {window}: {k}')
    print(f"\n[{name}] largest |device - oracle| / tolerance of the block means: {worst:.3f}")
    assert nx * ny > 0


def assert_same_frames(a, b, what, pick=None):
    sel = (lambda v: v[pick]) if pick is not None else (lambda v: v)
    assert sel(a['step']).tolist() == b['step'].tolist() and a['fields'] == b['fields'], what
    same_bits(sel(a['time']), b['time'], f'{what}: time')
    for k in a['fields']:
        same_bits(sel(a[k]), b[k], f'{what}: {k}')


SERIES_SPEC = dict(fields=('rho', 'p', 'h', 'tau_xz_top'), stride=(3, 5), reduce='mean', dtype='f8')


@pytest.mark.parametrize('name', ['48x37', '100x1'])
@pytest.mark.parametrize('every', [1, 3])
def test_series_of_a_run_equals_frame_now_after_every_update(hiplib, name, every):
    spec = dict(SERIES_SPEC, stride=(3, 5) if name == '48x37' else (7, 1))
    text = TEXT[name].replace('max_it: 100000', 'max_it: 10')
    from gapflow_amd import Problem
    rec, twin = quiet(Problem.from_string, text), quiet(Problem.from_string, text)
    rec.set_frames(every, **spec)
    quiet(rec.run)
    twin._pre_run()
    want, times = [], []
    for step in range(1, 11):
        twin.update()
        if step % every == 0:
            want.append(twin.frame_now(**spec))
            times.append(twin.simtime)
    s = rec.frames
    assert s['step'].tolist() == [k for k in range(1, 11) if k % every == 0] and s['fields'] == ('rho', 'p', 'h', 'tau_xz_top')
    assert s['reduce'] == 'mean' and s['stride'] == spec['stride']
    same_bits(s['time'], np.array(times), 'time against the stepped twin')
    assert s['time'].tolist() == times            # (a silent run keeps no history: test_run_writes_frames_nc holds the file against it)
    for i, w in enumerate(want):
        for k in s['fields']:
            same_bits(s[k][i], w[k], f'{name} every {every}: record {i}: {k}')
    same_bits(np.array(rec.q), np.array(twin.q), 'q of the armed run against the unarmed twin')
    now = rec.frame_now()
    if 10 % every == 0:
        for k in s['fields']:
            same_bits(now[k], s[k][-1], f'frame_now() of the armed frame against the last record: {k}')


@pytest.mark.parametrize('name', ['48x37', '100x1'])
def test_capacity_two_leaves_every_record(hiplib, name):
    ref, small = build(name), build(name)
    ref.set_frames(1, **SERIES_SPEC)
    small.set_frames(1, capacity=2, **SERIES_SPEC)
    ref._advance(7, honor_stop=False)
    small._advance(7, honor_stop=False)
    assert small.frames['step'].tolist() == list(range(1, 8))
    assert_same_frames(small.frames, ref.frames, 'capacity 2 against the default')
    same_bits(np.array(small.q), np.array(ref.q), 'final q')
    # in two calls, at stride 3 with a buffer of one record
    third = build(name)
    third.set_frames(3, capacity=1, **SERIES_SPEC)
    third._advance(5, honor_stop=False)
    assert third.frames['step'].tolist() == [3]
    third._advance(2, honor_stop=False)
    assert_same_frames(ref.frames, third.frames, 'stride 3, capacity 1 against stride 1', pick=[2, 5])


SMALL_SPEC = dict(fields=FIELDS, stride=(8, 1), reduce='mean', dtype='f8')
CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import test_gpu_frames as tf
states, out = np.load(sys.argv[1]), sys.argv[2]
p = tf.build('100x1')
p.set_frames(2, **tf.SMALL_SPEC)
p._advance(7, honor_stop=False)         # k_step2, one launch per step: the series of this form, against its own frame_now()
own = p.frames
assert own['step'].tolist() == [2, 4, 6]
twin = tf.build('100x1')
for step in range(1, 7):
    twin._advance(1, honor_stop=False)
    if step %% 2 == 0:
        now = twin.frame_now(**tf.SMALL_SPEC)
        for k in tf.FIELDS:
            tf.same_bits(own[k][step // 2 - 1], now[k], k)
res = {}
for key in states.files:                # the other form's states: the record is a function of the state alone
    p.q[...] = states[key]
    rec = p.frame_now(**tf.SMALL_SPEC)
    for k in tf.FIELDS:
        res[key + '_' + k] = rec[k]
np.savez(out, **res)
"""


def test_small_grid_batch_is_cut_at_the_recorded_steps_and_matches_the_launch_per_step_form(hiplib, tmp_path):
    """100 x 1, every = 2 on the one-workgroup kernel: pieces of 2, 2, 2, 1 against frame_now() behind single steps, and the run
    itself unchanged.  The same run with GPF_SMALL_GRID=0 (a child process: the switch is read once per process) goes through
    k_step2 with one recording launch behind each step; the two forms sum the step's scalars in different orders
    (tests/test_gpu_extras.py holds their states to 1e-10), so -- as tests/test_gpu_regions.py has it -- what must be equal there in
    every bit is the record of the SAME state: the child is handed the states this form recorded at and returns frame_now() of
    each, and checks its own batch against its own frame_now()."""
    import subprocess
    import sys
    rec, twin, plain = build('100x1'), build('100x1'), build('100x1')
    rec.set_frames(2, **SMALL_SPEC)
    rec._advance(7, honor_stop=False)
    plain._advance(7, honor_stop=False)
    s = rec.frames
    assert s['step'].tolist() == [2, 4, 6]
    same_bits(np.array(rec.q), np.array(plain.q), 'final q against the uncut batch')
    states = {}
    for step in range(1, 7):
        twin._advance(1, honor_stop=False)
        if step % 2 == 0:
            states[f's{step}'] = np.array(twin.q)
            now = twin.frame_now(**SMALL_SPEC)
            for k in FIELDS:
                same_bits(s[k][step // 2 - 1], now[k], f'step {step}: {k}')
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez(tmp_path / 'states.npz', **states)
    res = subprocess.run([sys.executable, '-c', CHILD % dict(root=os.path.dirname(here), tests=here), str(tmp_path / 'states.npz'), str(tmp_path / 'child.npz')],
                         env=dict(os.environ, GPF_SMALL_GRID='0'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(tmp_path / 'child.npz')
    for i, step in enumerate((2, 4, 6)):
        for k in FIELDS:
            same_bits(got[f's{step}_{k}'], s[k][i], f'step {step}: {k} through the launch-per-step form')


@pytest.mark.parametrize('name', ['48x37', '100x1'])
def test_rolled_back_step_leaves_no_record(hiplib, name):
    """tests/test_gpu_lines.py: test_rolled_back_step_leaves_no_record's way to an invalid state (an absurd time step)."""
    from gapflow_amd import _lib
    ref, p = build(name), build(name)
    for x in (ref, p):
        x.set_frames(1, **SERIES_SPEC)
        x._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_frames_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 0
    np.testing.assert_array_equal(p.q, good)
    assert_same_frames(p.frames, ref.frames, 'records before the rollback')
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.frame_now()
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.frame_now(fields=('rho',))


def test_other_series_and_frames_do_not_touch_each_other(hiplib):
    lines = [{'along': 'x'}, {'along': 'y', 'at': (3, 9), 'name': 'band'}]

    def run(frames, others):
        p = build('48x37')
        if frames:
            p.set_frames(2, **SERIES_SPEC)
        if others:
            p.set_integrals(3)
            p.set_lines(lines, 1)
            p.set_extrema(4)
        p._advance(5, honor_stop=False)
        p._advance(7, honor_stop=False)
        return p
    both, alone, rest = run(True, True), run(True, False), run(False, True)
    assert both.frames['step'].tolist() == [2, 4, 6, 8, 10, 12]
    assert_same_frames(both.frames, alone.frames, 'frames beside integrals, lines and extrema against frames alone')
    a, b = both.integrals, rest.integrals
    assert a.step.tolist() == b.step.tolist() == [3, 6, 9, 12]
    for k in a._fields:
        v, w = getattr(a, k), getattr(b, k)
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            same_bits(v, w, f'integrals.{k}')
    a, b = both.lines, rest.lines
    assert a['step'].tolist() == b['step'].tolist() == list(range(1, 13))
    for n in a['names']:
        for k in FIELDS:
            same_bits(a[n][k], b[n][k], f'lines: {n}.{k}')
    a, b = both.extrema, rest.extrema
    assert a.step.tolist() == b.step.tolist() == [4, 8, 12]
    for k in a._fields:
        v, w = getattr(a, k), getattr(b, k)
        if isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and v.tobytes() == w.tobytes(), f'extrema.{k}'
    same_bits(np.array(both.q), np.array(rest.q), 'final q')


def frame_spec(fields=0x0f, window=(0, 0, 0, 0), stride=(1, 1), reduce=0, dtype=0):
    from gapflow_amd import _lib
    s = _lib.GpfFrameSpec()
    s.fields, (s.ix0, s.ix1, s.iy0, s.iy1), (s.sx, s.sy), s.reduce, s.dtype = fields, window, stride, reduce, dtype
    return s


def test_refusals(hiplib):
    from gapflow_amd import Ensemble, Problem, _lib
    p = tp.build(GRID_48)
    lib, err = p._lib, p._lib.gpf_last_error
    nx, ny = p.grid['Nx'], p.grid['Ny']
    ok = C.byref(frame_spec())
    out = np.empty(9 * nx * ny)
    vp = out.ctypes.data_as(C.c_void_p)
    # the library's own checks
    assert lib.gpf_frames_set(None, 1, ok, 0) == -1 and b'null handle' in err()
    assert lib.gpf_frames_set(p._h, 1, None, 0) == -1 and b'null spec' in err()
    assert lib.gpf_frames_set(p._h, 0, ok, 0) == -1 and b'every >= 1' in err()
    assert lib.gpf_frames_set(p._h, 1, ok, -1) == -1 and b'capacity >= 1' in err()
    for mask in (0, 1 << 9, -1):
        assert lib.gpf_frames_set(p._h, 1, C.byref(frame_spec(fields=mask)), 0) == -1 and b'non-empty mask of the nine fields' in err()
    for w in ((0, nx, 1, ny), (1, nx + 1, 1, ny), (1, nx, 1, ny + 1), (9, 3, 1, ny), (1, nx, 5, 2), (1, 0, 0, 0)):
        assert lib.gpf_frames_set(p._h, 1, C.byref(frame_spec(window=w)), 0) == -1 and b'window (' in err(), w
    for st in ((0, 1), (1, 0), (65, 1), (1, 65)):
        assert lib.gpf_frames_set(p._h, 1, C.byref(frame_spec(stride=st)), 0) == -1 and b'must lie within 1..64' in err(), st
    assert lib.gpf_frames_set(p._h, 1, C.byref(frame_spec(reduce=2)), 0) == -1 and b'reduce must be 0 (sample) or 1 (mean)' in err()
    assert lib.gpf_frames_set(p._h, 1, C.byref(frame_spec(dtype=2)), 0) == -1 and b'dtype must be 0 (f8) or 1 (f4)' in err()
    assert lib.gpf_frames_read(p._h, None, 0, None, None) == -5 and b'no frames are armed' in err()
    assert lib.gpf_frames_read(None, None, 0, None, None) == -1
    assert lib.gpf_frames_clear(None) == -1 and lib.gpf_frames_now(None, ok, vp, out.nbytes) == -1
    assert lib.gpf_frames_now(p._h, ok, None, out.nbytes) == -1 and b'null argument' in err()
    assert lib.gpf_frames_now(p._h, None, vp, out.nbytes) == -5 and b'no frames are armed' in err()
    assert lib.gpf_frames_now(p._h, C.byref(frame_spec(stride=(0, 1))), vp, out.nbytes) == -1 and b'must lie within' in err()
    assert lib.gpf_frames_now(p._h, ok, vp, 4 * nx * ny * 8 - 1) == -1 and f'room for {4 * nx * ny * 8} bytes'.encode() in err()
    mx, my, nbytes = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    _lib.check(lib.gpf_frames_shape(p._h, C.byref(frame_spec(fields=0x111, window=(5, 41, 4, 33), stride=(3, 5), reduce=1, dtype=1)),
                                    C.byref(mx), C.byref(my), C.byref(nbytes)))
    assert (mx.value, my.value, nbytes.value) == (13, 6, 3 * 13 * 6 * 4)
    _lib.check(lib.gpf_frames_shape(p._h, ok, None, None, None))
    assert lib.gpf_frames_shape(None, ok, None, None, None) == -1 and lib.gpf_frames_shape(p._h, None, None, None, None) == -1
    ms = C.c_double(0.)
    assert lib.gpf_frames_time(p._h, 2, 1, C.byref(ms)) == -5 and b'mode 1 needs armed frames' in err()
    assert lib.gpf_frames_time(p._h, 2, 1, None) == -1 and lib.gpf_frames_time(None, 2, 1, C.byref(ms)) == -1
    _lib.check(lib.gpf_frames_set(p._h, 1, C.byref(frame_spec(stride=(8, 8), reduce=1, dtype=1)), 3))
    assert lib.gpf_frames_now(p._h, None, vp, 4 * 6 * 5 * 4 - 1) == -1 and f'room for {4 * 6 * 5 * 4} bytes'.encode() in err()
    _lib.check(lib.gpf_frames_now(p._h, None, vp, out.nbytes))
    assert lib.gpf_frames_time(p._h, 4, 1, C.byref(ms)) == -1 and b'more records than the buffer holds (3 at stride 1)' in err()
    _lib.check(lib.gpf_frames_time(p._h, 3, 1, C.byref(ms)))
    assert ms.value > 0
    have = C.c_int64(-1)
    _lib.check(lib.gpf_frames_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 3
    _lib.check(lib.gpf_frames_time(p._h, 3, 0, C.byref(ms)))
    _lib.check(lib.gpf_frames_clear(p._h))
    # Python's checks
    for bad in (dict(fields=('rho', 'q')), dict(window=(0, 5, 1, 5)), dict(window=(1, nx + 1, 1, ny)), dict(window=(9, 3, 1, 5)), dict(stride=(0, 1)),
                dict(stride=(1, 65)), dict(reduce='max'), dict(dtype='f2'), dict(capacity=0), dict(every=0), dict(keep=1)):
        with pytest.raises(ValueError, match='frames'):
            p.set_frames(**bad)
    with pytest.raises(ValueError, match='frame_now'):
        p.frame_now(stride=(0, 1))
    with pytest.raises(ValueError, match='frame_now'):
        p.frame_now(capacity=2)
    with pytest.raises(RuntimeError, match='no frames are set'):
        p.frame_now()
    assert p.frames is None
    # a slab handle: this problem's configuration with a halo row
    cfg = _lib.GpfConfig.from_buffer_copy(p._cfg)
    cfg.halo_lo = 1
    slab = C.c_void_p()
    assert lib.gpf_create(C.byref(cfg), C.byref(slab)) == 0
    try:
        assert lib.gpf_frames_set(slab, 1, ok, 0) == -5 and b'this handle is a slab; frames are not available on slabs' in err()
    finally:
        lib.gpf_destroy(slab)
    # an open stage-wise step
    _lib.check(lib.gpf_open_step(p._h))
    assert lib.gpf_frames_set(p._h, 1, ok, 0) == -5 and b'stage-wise step is open' in err()
    assert lib.gpf_frames_clear(p._h) == -5 and b'stage-wise step is open' in err()
    assert lib.gpf_frames_now(p._h, ok, vp, out.nbytes) == -5 and b'stage-wise step is open' in err()
    for i in range(2):
        _lib.check(lib.gpf_stage_closures(p._h))
        _lib.check(lib.gpf_stage_advance(p._h, i))
    sc = _lib.GpfScalars()
    _lib.check(lib.gpf_close_step(p._h, C.byref(sc)))
    # gpf_close_step records nothing
    p.set_frames(1)
    _lib.check(lib.gpf_open_step(p._h))
    for i in range(2):
        _lib.check(lib.gpf_stage_closures(p._h))
        _lib.check(lib.gpf_stage_advance(p._h, i))
    _lib.check(lib.gpf_close_step(p._h, C.byref(sc)))
    _lib.check(lib.gpf_frames_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 0
    # shear thinning
    t = tp.build(THINNING)
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.set_frames()
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.frame_now(fields=('rho',))
    assert t._lib.gpf_frames_set(t._h, 1, ok, 0) == -1 and b'shear thinning' in err()
    assert t._lib.gpf_frames_now(t._h, ok, vp, out.nbytes) == -1 and b'shear thinning' in err()
    # an elastic gap
    e = tp.build(ELASTIC)
    with pytest.raises(NotImplementedError, match='elastic gap'):
        e.set_frames()
    assert e._lib.gpf_frames_set(e._h, 1, ok, 0) == -1 and b'elastic handle' in err()
    # surrogate closures
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = quiet(Problem.from_string, SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            g.set_frames()
        quiet(g._pre_run)
        assert g._lib.gpf_frames_set(g._h, 1, ok, 0) == -1 and b'surrogate' in err()
    # an armed member of an ensemble: member and reason named, by the package and by the library
    members = [tp.build(JOURNAL_1D), tp.build(JOURNAL_1D.replace('eps: 0.7', 'eps: 0.5'))]
    members[1].set_frames()
    with pytest.raises(NotImplementedError, match='member 1: frames are armed'):
        Ensemble(members)
    handles = (C.c_void_p * 2)(*[m._h.value for m in members])
    ens = C.c_void_p()
    assert lib.gpf_ensemble_create(handles, 2, C.byref(ens)) == -1
    assert b'member 1: frames are armed on it (they cut the batch per member; gpf_frames_clear, or step it alone)' in err()
    members[1].clear_frames()
    made = Ensemble(members)
    members[0].set_frames()
    with pytest.raises(NotImplementedError, match='member 0: .*frames are armed'):
        made.step(3)


def run_yaml(out, silent, max_it=12, more=''):
    options = (f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, frames: 3, "
               f"frame_spec: {{fields: [p, rho, tau_xz_bot], window: [3, 98, 1, 1], stride: [8, 1], reduce: mean{more}}}}}")
    return JOURNAL_1D.replace("options: {silent: True}", options).replace('max_it: 100000', f'max_it: {max_it}')


def test_run_writes_frames_nc(hiplib, tmp_path):
    from scipy.io import netcdf_file
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False))
    twin = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True))
    assert p._frames_keep is False and twin._frames_keep is True
    quiet(p.run)
    quiet(twin.run)
    s = twin.frames
    assert s['step'].tolist() == [3, 6, 9, 12] and s['fields'] == ('rho', 'p', 'tau_xz_bot') and s['rho'].shape == (4, 12, 1) and s['rho'].dtype == np.float32
    kept = p.frames
    assert kept['step'].shape == (0,) and kept['rho'].shape == (0, 12, 1) and kept['rho'].dtype == np.float32      # keep=False: the file has them all
    with netcdf_file(os.path.join(p.outdir, 'frames.nc'), 'r', mmap=False) as f:
        assert f.version_byte == 2
        assert f.dimensions['frame'] is None and f.dimensions['nx'] == 12 and f.dimensions['ny'] == 1
        assert sorted(f.variables) == sorted(['step', 'time', 'x', 'y', 'rho', 'p', 'tau_xz_bot'])
        assert f.variables['step'].data.dtype.newbyteorder('=') == np.dtype('i4') and f.variables['step'][:].tolist() == [3, 6, 9, 12]
        same_bits(f.variables['time'][:].astype(np.float64), s['time'], 'time')
        same_bits(f.variables['x'][:].astype(np.float64), s['x'], 'x')
        same_bits(f.variables['y'][:].astype(np.float64), s['y'], 'y')
        for k in s['fields']:
            v = f.variables[k]
            assert v.dimensions == ('frame', 'nx', 'ny') and v.data.dtype.newbyteorder('=') == np.dtype('f4')
            same_bits(v[:].astype(np.float32), s[k], f'frames.nc: {k}')
        hist = dict(zip(p.history['step'], p.history['time']))      # the rows of history.csv: steps 0, 5, 10, 12
        assert 12 in hist and hist[12] == f.variables['time'][:].tolist()[-1]
        assert f.window.tolist() == [3, 98, 1, 1] and f.stride.tolist() == [8, 1] and f.reduce == b'mean'
    # keep=True on a problem that is not silent: the file and the memory
    k = quiet(Problem.from_string, run_yaml(tmp_path / 'kept', False).replace('frames: 3, ', ''))
    k.set_frames(3, fields=('p', 'rho', 'tau_xz_bot'), window=(3, 98, 1, 1), stride=(8, 1), reduce='mean', keep=True)
    quiet(k.run)
    assert_same_frames(k.frames, s, 'keep=True beside the file')
    with netcdf_file(os.path.join(k.outdir, 'frames.nc'), 'r', mmap=False) as f:
        same_bits(f.variables['p'][:].astype(np.float32), s['p'], 'frames.nc of the keep=True run: p')


def test_restored_problem_rearms_and_records_from_the_restart_step(hiplib, tmp_path):
    from gapflow_amd import Problem
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000, more=', dtype: f8, capacity: 2'))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(7, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.frames['step'].shape == (0,) and b.frames['fields'] == ('rho', 'p', 'tau_xz_bot') and b.frames['p'].shape == (0, 12, 1)
    assert b.frames['p'].dtype == np.float64 and b.frames['reduce'] == 'mean' and b.frames['window'] == (3, 98, 1, 1)
    b._advance(7, honor_stop=False)
    assert a.frames['step'].tolist() == [3, 6, 9, 12] and b.frames['step'].tolist() == [6, 9, 12]
    assert_same_frames(a.frames, b.frames, 'continued against restored', pick=[1, 2, 3])
    # _pre_run starts a new series; init_from does, too
    a._pre_run()
    assert a.frames['step'].shape == (0,)
    a._advance(3, honor_stop=False)
    assert a.frames['step'].tolist() == [3]
    a.init_from(b)
    assert a.frames['step'].shape == (0,) and a.step == 0
    # frames armed from code do not enter the options and do not survive a restore
    c = build('100x1')
    c.set_frames(1)
    c._advance(2, honor_stop=False)
    c.save_checkpoint(str(tmp_path / 'd.gpf'))
    assert quiet(Problem.from_checkpoint, str(tmp_path / 'd.gpf')).frames is None
    b.clear_frames()
    assert b.frames is None
