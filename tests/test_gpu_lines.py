"""Line profiles (gpf_lines_*, Problem.set_lines / lines / film_lines, options.lines): the nine fields rho, jx, jy, p, h and the four
wall shear stresses along interior rows and columns, at one index or averaged over a band, recorded on the device while gpf_step
advances whole batches.

Yardsticks.  A second, identical Problem advanced by update() one step at a time, with probes armed on the lines' cells and q read
after every step: a single-index line's rho / jx / jy equal that q, its h the gap, its p the probe's p, all in every bit; its four
stresses agree with oracle/closures.py (stress_bottom / stress_top with slip="top", as tests/test_gpu_integrals.py evaluates them)
on the downloaded state at rtol 1e-12 + atol 1e-13 max|field| -- the per-cell tolerance tests/test_gpu_parity.py:
test_closure_fields_match_reference_outputs holds cell_fields to.  A band equals, in every bit, the sum and division that
csrc/lines.hpp states, restated here in NumPy over the single-index lines of the same state.  Everything else is held bit for
bit: a record is a pure function of the state, and recording only reads.

Grids: 45 x 37 asperity, Dirichlet / Neumann in x and periodic in y (k_step2; odd sizes; 45 rows are chunks of 32 + 13); 20 x 70
journal (k_step2; 70 columns: a lane of the band along x walks on to a second cell); the 1-D journal 100 x 1 (k_small_steps, where
the batch is cut at the recorded steps)."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest

import test_gpu_probes as tp
from test_gpu_probes import JOURNAL_1D, SCALARS, SURROGATE, THINNING, assert_bitwise, assert_same_scalars, quiet, scalars_of
from test_gpu_weighted import ELASTIC

pytestmark = pytest.mark.gpu

FIELDS = ('rho', 'jx', 'jy', 'p', 'h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')
ASPERITY = """
options: {silent: True}
grid: {Nx: 45, Ny: 37, Lx: 0.009, Ly: 0.0074, %s, xE_D: 877.7007, xW_D: 876.}
geometry: {type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.05}
numerics: {CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1e-14, dt: 2.e-9, max_it: 100000}
properties: {EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}
""" % tp.DN
JOURNAL_2D = """
options: {silent: True}
grid: {Nx: 20, Ny: 70, dx: 1.e-5, dy: 1.e-5}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.02}
numerics: {CFL: 0.5, adaptive: 1, tol: 1.e-14, max_it: 100000}
properties: {EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007, P0: 101325., C1: 3.5e10, C2: 1.23}
"""
TEXT = {'asperity': ASPERITY, 'journal-2d': JOURNAL_2D, 'journal-1d': JOURNAL_1D}
NAMES = list(TEXT)
NSTEPS = 4
# single-index lines: the first and the last column / row and the default centre (journal-2d: 200 of the 256 cells probes take)
SINGLES = {'asperity': [('x', 1), ('x', 37), ('x', None), ('y', 1), ('y', 45), ('y', None)],
           'journal-2d': [('x', 1), ('x', 70), ('x', None), ('y', 1), ('y', 20)],
           'journal-1d': [('x', 1), ('x', None), ('y', 1), ('y', 100), ('y', None)]}
# bands: (3, 9) and the whole extent both ways -- (1, 70) along x wraps the 64 lanes, (1, 45) along y is chunks of 32 + 13
BANDS = {'asperity': [('x', (3, 9)), ('x', (1, 37)), ('y', (3, 9)), ('y', (1, 45)), ('y', (14, 45)), ('x', (36, 37))],
         'journal-2d': [('x', (3, 9)), ('x', (1, 70)), ('x', (6, 70)), ('y', (3, 9)), ('y', (1, 20))],
         'journal-1d': [('y', (3, 9)), ('y', (1, 100)), ('y', (1, 33)), ('y', (69, 100))]}


def entries(pairs):
    return [{'along': a, 'at': at, 'name': f'{a}{k}'} for k, (a, at) in enumerate(pairs)]


def cells_of(along, at, nx, ny):
    """The ghosted-index cells of a single-index line; at None: the reference's centre line, ny // 2 of the ghosted shape."""
    if at is None:
        at = (ny + 2) // 2 if along == 'x' else (nx + 2) // 2
    return [(ix, at) for ix in range(1, nx + 1)] if along == 'x' else [(at, iy) for iy in range(1, ny + 1)]


def oracle_stresses(p, q):
    """tau_xz_bot, tau_yz_bot, tau_xz_top, tau_yz_top over the ghosted grid, as tests/test_gpu_integrals.py: oracle_record has them."""
    from gapflow_amd import _lib
    from oracle import closures as ocl
    topo, Ls = np.array(p.topo.full[:3]), np.array(p._extra[0])
    prop = dict(_lib.EOS_DEFAULTS[p.prop['EOS']], **p.prop)
    pr = ocl.eos_pressure(q[0], prop)
    eta = ocl.piezoviscosity(pr, p.prop['shear'], p.prop['piezo']) if 'piezo' in p.prop else p.prop['shear']
    bot = ocl.stress_bottom(q, topo, p.geo['U'], p.geo['V'], eta, p.prop['bulk'], Ls, slip="top")
    top = ocl.stress_top(q, topo, p.geo['U'], p.geo['V'], eta, p.prop['bulk'], Ls, slip="top")
    return [np.broadcast_to(t, q[0].shape) for t in (bot[4], bot[3], top[4], top[3])]


@functools.lru_cache(maxsize=None)
def case_runs(name):
    """One recorded batch of NSTEPS steps (every = 1) of the single-index lines, the twin stepped one update() at a time with probes
    on the lines' cells, and the same batch without lines; computed once per case and only read by the tests.  `rec` stays at its
    final state for film_lines."""
    rec, twin, plain = tp.build(TEXT[name]), tp.build(TEXT[name]), tp.build(TEXT[name])
    nx, ny = rec.grid['Nx'], rec.grid['Ny']
    lines = entries(SINGLES[name])
    rec.set_lines(lines)
    log = rec._advance(NSTEPS, honor_stop=False)
    plain_log = plain._advance(NSTEPS, honor_stop=False)
    cells = [c for a, at in SINGLES[name] for c in cells_of(a, at, nx, ny)]
    twin.set_probes(cells, pressure=True)
    qs, times = [], []
    for _ in range(NSTEPS):
        twin.update()
        qs.append(twin.q.copy())
        times.append(twin.simtime)
    return dict(rec=rec, lines=lines, series=rec.lines, cells=cells, qs=qs, times=times, probes=twin.probes, twin=twin,
                q=rec.q.copy(), scalars=scalars_of(rec), log=[tuple(getattr(e, k) for k in SCALARS) for e in log],
                plain_q=plain.q.copy(), plain_scalars=scalars_of(plain), plain_log=[tuple(getattr(e, k) for k in SCALARS) for e in plain_log])


@pytest.mark.parametrize('name', NAMES)
def test_single_index_lines_equal_reading_the_state(hiplib, name):
    r = case_runs(name)
    s, twin = r['series'], r['twin']
    nx, ny = twin.grid['Nx'], twin.grid['Ny']
    assert s['names'] == tuple(e['name'] for e in r['lines']) and s['step'].tolist() == list(range(1, NSTEPS + 1))
    assert_bitwise(s['time'], r['times'], 'time')
    assert r['probes'].step.tolist() == s['step'].tolist()
    gap = np.array(twin.topo.full[0])
    at, worst = 0, 0.0
    for e, (along, where) in zip(r['lines'], SINGLES[name]):
        cells = cells_of(along, where, nx, ny)
        ix, iy = np.array(cells).T
        got = s[e['name']]
        assert sorted(got) == sorted(FIELDS) and all(got[f].shape == (NSTEPS, len(cells)) for f in FIELDS), e
        for k in range(NSTEPS):
            q = r['qs'][k]
            for c, f in enumerate(('rho', 'jx', 'jy')):
                assert_bitwise(got[f][k], q[c][ix, iy], f"{e['name']} step {k + 1}: {f} against the downloaded q")
            assert_bitwise(got['h'][k], gap[ix, iy], f"{e['name']} step {k + 1}: h against the gap")
            assert_bitwise(got['p'][k], r['probes'].p[k, at:at + len(cells)], f"{e['name']} step {k + 1}: p against the probes' p")
            for f, ref in zip(FIELDS[5:], oracle_stresses(twin, q)):
                scale = np.abs(ref[1:-1, 1:-1]).max()
                np.testing.assert_allclose(got[f][k], ref[ix, iy], rtol=1e-12, atol=1e-13 * scale, err_msg=f"{e['name']} step {k + 1}: {f}")
                tol = 1e-12 * np.abs(ref[ix, iy]) + 1e-13 * scale
                worst = max(worst, (np.abs(got[f][k] - ref[ix, iy])[tol > 0] / tol[tol > 0]).max(initial=0.0))
        at += len(cells)
    assert r['probes'].cells.tolist() == [list(c) for c in r['cells']] and at == len(r['cells'])
    print(f"\n[{name}] largest |device - oracle| / tolerance of the wall stresses: {worst:.3f}")
    assert_bitwise(r['q'], r['qs'][-1], 'final q against the stepped twin')


@functools.lru_cache(maxsize=None)
def all_singles(name):
    """The nine fields on the whole interior, (9, Nx, Ny), from the single-index lines of case_runs(name)'s final state: every
    column as a line along x, eight per film_lines call -- and once more from every row as a line along y."""
    p = case_runs(name)['rec']
    nx, ny = p.grid['Nx'], p.grid['Ny']
    out = {}
    for along, n in (('x', ny), ('y', nx)):
        F = np.empty((9, nx, ny))
        for first in range(1, n + 1, 8):
            idx = list(range(first, min(first + 8, n + 1)))
            got = p.film_lines(lines=[{'along': along, 'at': i, 'name': f'i{i}'} for i in idx])
            for i in idx:
                for k, f in enumerate(FIELDS):
                    if along == 'x':
                        F[k, :, i - 1] = got[f'i{i}'][f]
                    else:
                        F[k, i - 1, :] = got[f'i{i}'][f]
        out[along] = F
    return out


def band_along_x(F, i0, i1):
    """csrc/lines.hpp, restated: lane l adds the columns i0 + l, i0 + l + 64, ... ascending from +0.0; the 64 lanes fold 32, 16, .. 1
    apart; lane 0 divides by n."""
    lanes = np.zeros((64,) + F.shape[:2])
    for lane in range(64):
        for iy in range(i0 + lane, i1 + 1, 64):
            lanes[lane] = lanes[lane] + F[:, :, iy - 1]
    s = 32
    while s >= 1:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return lanes[0] / np.float64(i1 - i0 + 1)


def band_along_y(F, i0, i1):
    """csrc/lines.hpp, restated: chunks of 32 consecutive rows from i0, each added ascending from +0.0; the chunk sums added
    ascending from +0.0; divided by n."""
    total = np.zeros((F.shape[0], F.shape[2]))
    for first in range(i0, i1 + 1, 32):
        part = np.zeros_like(total)
        for ix in range(first, min(first + 31, i1) + 1):
            part = part + F[:, ix - 1, :]
        total = total + part
    return total / np.float64(i1 - i0 + 1)


@pytest.mark.parametrize('name', NAMES)
def test_band_equals_the_restated_sum_of_the_single_index_lines(hiplib, name):
    p = case_runs(name)['rec']
    F = all_singles(name)
    assert_bitwise(F['x'], F['y'], 'the interior from lines along x and from lines along y')
    assert np.all(np.isfinite(F['x']))
    lines = entries(BANDS[name])
    got = p.film_lines(lines=lines)
    assert p.lines['names'] == tuple(e['name'] for e in case_runs(name)['lines'])       # nothing was armed or disarmed
    for e, (along, (i0, i1)) in zip(lines, BANDS[name]):
        want = band_along_x(F['x'], i0, i1) if along == 'x' else band_along_y(F['x'], i0, i1)
        for k, f in enumerate(FIELDS):
            assert_bitwise(got[e['name']][f], want[k], f"{name}: band {along} {i0}..{i1}: {f}")
    # a pair (i, i) is the single-index line: no addition, no division
    one = p.film_lines(lines=[{'along': 'y', 'at': (2, 2), 'name': 'pair'}])['pair']
    for k, f in enumerate(FIELDS):
        assert_bitwise(one[f], F['x'][k, 1, :], f"(2, 2) along y: {f}")


SERIES = {'asperity': [('x', None), ('y', (1, 45)), ('x', (3, 9)), ('y', 7)],
          'journal-1d': [('x', None), ('y', (1, 100)), ('y', 50)]}


def assert_same_series(a, b, what, pick=None):
    """Bitwise; `pick`: indices of a's records to hold against all of b's."""
    sel = (lambda v: v[pick]) if pick is not None else (lambda v: v)
    assert sel(a['step']).tolist() == b['step'].tolist() and a['names'] == b['names'], what
    assert_bitwise(sel(a['time']), b['time'], f"{what}: time")
    for n in a['names']:
        for f in FIELDS:
            assert_bitwise(sel(a[n][f]), b[n][f], f"{what}: {n}.{f}")


def armed(name, every=1, capacity=None):
    p = tp.build(TEXT[name])
    p.set_lines(entries(SERIES[name]), every, capacity)
    return p


@functools.lru_cache(maxsize=None)
def series_runs(name):
    rec, plain = armed(name), tp.build(TEXT[name])
    log = rec._advance(12, honor_stop=False)
    plain_log = plain._advance(12, honor_stop=False)
    return dict(series=rec.lines, q=rec.q.copy(), scalars=scalars_of(rec), log=[tuple(getattr(e, k) for k in SCALARS) for e in log],
                plain_q=plain.q.copy(), plain_scalars=scalars_of(plain), plain_log=[tuple(getattr(e, k) for k in SCALARS) for e in plain_log])


@pytest.mark.parametrize('name', list(SERIES))
def test_series_does_not_depend_on_the_batches(hiplib, name):
    """12 steps as one call, as 12 calls, and with a buffer of two records (gpf_step cuts its batches at two records) give the same
    series and the same run; a stride of 3 gives the matching subset, with a buffer of two records as well."""
    ref = series_runs(name)
    assert ref['series']['step'].tolist() == list(range(1, 13))
    single = armed(name)
    for _ in range(12):
        single._advance(1, honor_stop=False)
    assert_same_series(single.lines, ref['series'], '12 calls against one')
    small = armed(name, capacity=2)
    small._advance(12, honor_stop=False)
    assert_same_series(small.lines, ref['series'], 'capacity 2 against the default')
    one = armed(name, capacity=1)
    one._advance(5, honor_stop=False)
    one._advance(7, honor_stop=False)
    assert_same_series(one.lines, ref['series'], 'capacity 1 in two calls against the default')
    for p in (single, small, one):
        assert_bitwise(p.q, ref['q'], 'final q')
        assert_same_scalars(scalars_of(p), ref['scalars'], 'final scalars')
    for capacity in (None, 2):
        third = armed(name, every=3, capacity=capacity)
        third._advance(5, honor_stop=False)
        assert third.lines['step'].tolist() == [3]
        third._advance(7, honor_stop=False)
        assert_same_series(ref['series'], third.lines, f'stride 3 (capacity {capacity}) against stride 1', pick=[2, 5, 8, 11])
        assert_bitwise(third.q, ref['q'], 'final q at stride 3')
    now = single.film_lines()
    for n in ref['series']['names']:
        for f in FIELDS:
            assert_bitwise(now[n][f], ref['series'][n][f][-1], f"film_lines() against the last record: {n}.{f}")


@pytest.mark.parametrize('name', NAMES)
def test_recording_leaves_the_run_unchanged(hiplib, name):
    for r in [case_runs(name)] + ([series_runs(name)] if name in SERIES else []):
        assert_bitwise(r['q'], r['plain_q'], 'final q with and without lines')
        assert_same_scalars(r['scalars'], r['plain_scalars'], 'final scalars')
        assert len(r['log']) == len(r['plain_log'])
        for i, (a, b) in enumerate(zip(r['log'], r['plain_log'])):
            assert_same_scalars(a, b, f"scalar record of step {i + 1}")


def run_yaml(out, silent, max_it=12):
    options = (f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, lines: 3, "
               f"line_list: [{{along: x}}, {{along: y, at: [1, 100], name: band}}, {{along: y, at: 50, name: mid}}]}}")
    return JOURNAL_1D.replace("options: {silent: True}", options).replace('max_it: 100000', f'max_it: {max_it}')


def test_history_and_q_of_a_run_are_those_of_the_run_without_lines(hiplib, tmp_path):
    from gapflow_amd import Problem
    with_lines = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True))
    without = quiet(Problem.from_string, JOURNAL_1D.replace('max_it: 100000', 'max_it: 12'))
    quiet(with_lines.run)
    quiet(without.run)
    assert with_lines.lines['step'].tolist() == [3, 6, 9, 12] and without.lines is None
    assert_bitwise(with_lines.q, without.q, 'q after run()')
    assert sorted(with_lines.history) == sorted(without.history)
    for k in without.history:
        assert_bitwise(with_lines.history[k], without.history[k], f'history: {k}')


@pytest.mark.parametrize('name', list(SERIES))
def test_rolled_back_step_leaves_no_record(hiplib, name):
    """tests/test_gpu_regions.py: test_rolled_back_step_leaves_no_record's way to an invalid state (an absurd time step): the scalar
    log keeps its entry for the invalid step, the series ends one entry before it, and film_lines() refuses the state."""
    from gapflow_amd import _lib
    p = armed(name)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_lines_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 0
    np.testing.assert_array_equal(p.q, good)
    assert_same_series(series_runs(name)['series'], p.lines, 'records before the rollback', pick=[0, 1, 2])
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.film_lines()
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.film_lines(lines=[{'along': 'x'}])


def test_run_writes_lines_npz_and_a_restored_problem_rearms(hiplib, tmp_path):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'lines.npz'))
    names = ['l0', 'band', 'mid']
    assert sorted(f.files) == sorted(['step', 'time', 'names', 'along', 'at'] + [f'{n}.{q}' for n in names for q in FIELDS])
    assert f['names'].tolist() == names and f['step'].tolist() == [3, 6, 9, 12]
    assert f['along'].tolist() == ['x', 'y', 'y'] and f['at'].tolist() == [[1, 1], [1, 100], [50, 50]]
    assert f['l0.p'].shape == (4, 100) and f['band.p'].shape == (4, 1) and f['mid.rho'].shape == (4, 1)
    ref = series_runs('journal-1d')['series']           # the same problem and lines (named x0, y1, y2 there), every = 1
    assert_bitwise(f['time'], ref['time'][[2, 5, 8, 11]], 'run() at stride 3 against the batch at stride 1: time')
    for n, m in zip(names, ref['names']):
        for q in FIELDS:
            assert_bitwise(f[f'{n}.{q}'], ref[m][q][[2, 5, 8, 11]], f"run() at stride 3 against the batch at stride 1: {n}.{q}")
    # checkpoints do not carry the series: the restored problem re-arms from its options and records from the restart step
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(7, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.lines['step'].shape == (0,) and b.lines['names'] == ('l0', 'band', 'mid') and b.lines['band']['p'].shape == (0, 1)
    b._advance(7, honor_stop=False)
    assert a.lines['step'].tolist() == [3, 6, 9, 12] and b.lines['step'].tolist() == [6, 9, 12]
    assert_same_series(a.lines, b.lines, 'continued against restored', pick=[1, 2, 3])
    # _pre_run starts a new series
    a._pre_run()
    assert a.lines['step'].shape == (0,)
    # lines armed from code do not enter the options and do not survive a restore
    c = armed('journal-1d')
    c._advance(2, honor_stop=False)
    c.save_checkpoint(str(tmp_path / 'd.gpf'))
    assert quiet(Problem.from_checkpoint, str(tmp_path / 'd.gpf')).lines is None
    b.clear_lines()
    assert b.lines is None


def line_array(*lines):
    from gapflow_amd import _lib
    arr = (_lib.GpfLine * len(lines))()
    for a, (along, i0, i1) in zip(arr, lines):
        a.along, a.i0, a.i1 = along, i0, i1
    return arr


def test_refusals(hiplib):
    from gapflow_amd import Ensemble, Problem, _lib
    p = tp.build(ASPERITY)
    nx, ny = p.grid['Nx'], p.grid['Ny']
    ok = line_array((0, 0, 0))
    err = p._lib.gpf_last_error
    out = np.empty(9 * 8 * 45)
    # the library's own checks
    for K in (0, 9):
        assert p._lib.gpf_lines_set(p._h, 1, K, line_array(*[(0, 1, 1)] * 9), 0) == -1 and f'1 to 8 lines required, got {K}'.encode() in err()
    assert p._lib.gpf_lines_set(p._h, 0, 1, ok, 0) == -1 and b'every >= 1' in err()
    assert p._lib.gpf_lines_set(p._h, 1, 1, ok, -1) == -1 and b'capacity >= 1' in err()
    assert p._lib.gpf_lines_set(p._h, 1, 1, None, 0) == -1 and b'null lines' in err()
    for along in (-1, 2):
        assert p._lib.gpf_lines_set(p._h, 1, 2, line_array((0, 1, 1), (along, 1, 1)), 0) == -1 and b'line 1: along must be 0 (x) or 1 (y)' in err()
    for bad in ((0, 0, 5), (0, 1, ny + 1), (0, 9, 3), (1, 1, nx + 1), (1, 0, 1), (0, ny + 1, ny + 1), (1, 5, 0)):
        assert p._lib.gpf_lines_set(p._h, 1, 1, line_array(bad), 0) == -1 and b'line 0: indices' in err(), bad
    assert p._lib.gpf_lines_read(p._h, None, 0, None, None) == -5 and b'no lines are armed' in err()
    assert p._lib.gpf_lines_now(p._h, 0, None, _lib.as_dp(out), out.size) == -5 and b'no lines are armed' in err()
    assert p._lib.gpf_lines_now(p._h, 1, line_array((0, 1, ny + 1)), _lib.as_dp(out), out.size) == -1 and b'line 0: indices' in err()
    assert p._lib.gpf_lines_now(p._h, 1, ok, _lib.as_dp(out), 9 * nx - 1) == -1 and f'room for {9 * nx} doubles'.encode() in err()
    ms = C.c_double(0.)
    assert p._lib.gpf_lines_time(p._h, 2, 1, C.byref(ms)) == -5 and b'mode 1 needs armed lines' in err()
    _lib.check(p._lib.gpf_lines_set(p._h, 1, 2, line_array((0, 0, 0), (1, 1, nx)), 3))
    assert p._lib.gpf_lines_now(p._h, 0, None, _lib.as_dp(out), 9 * (nx + ny) - 1) == -1 and f'room for {9 * (nx + ny)} doubles'.encode() in err()
    _lib.check(p._lib.gpf_lines_now(p._h, 0, None, _lib.as_dp(out), out.size))
    assert np.all(np.isfinite(out[:9 * (nx + ny)]))
    assert p._lib.gpf_lines_time(p._h, 4, 1, C.byref(ms)) == -1 and b'more records than the buffer holds (3 at stride 1)' in err()
    _lib.check(p._lib.gpf_lines_time(p._h, 3, 1, C.byref(ms)))
    assert ms.value > 0
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_lines_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 3
    _lib.check(p._lib.gpf_lines_clear(p._h))
    # an open stage-wise step
    _lib.check(p._lib.gpf_open_step(p._h))
    assert p._lib.gpf_lines_set(p._h, 1, 1, ok, 0) == -5 and b'stage-wise step is open' in err()
    assert p._lib.gpf_lines_clear(p._h) == -5 and b'stage-wise step is open' in err()
    assert p._lib.gpf_lines_now(p._h, 1, ok, _lib.as_dp(out), out.size) == -5 and b'stage-wise step is open' in err()
    for i in range(2):
        _lib.check(p._lib.gpf_stage_closures(p._h))
        _lib.check(p._lib.gpf_stage_advance(p._h, i))
    sc = _lib.GpfScalars()
    _lib.check(p._lib.gpf_close_step(p._h, C.byref(sc)))
    # shear thinning
    t = tp.build(THINNING)
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.set_lines([{'along': 'x'}])
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.film_lines(lines=[{'along': 'x'}])
    assert t._lib.gpf_lines_set(t._h, 1, 1, ok, 0) == -1 and b'shear thinning' in t._lib.gpf_last_error()
    assert t._lib.gpf_lines_now(t._h, 1, ok, _lib.as_dp(out), out.size) == -1 and b'shear thinning' in t._lib.gpf_last_error()
    # an elastic gap
    e = tp.build(ELASTIC)
    with pytest.raises(NotImplementedError, match='elastic gap'):
        e.set_lines([{'along': 'x'}])
    assert e._lib.gpf_lines_set(e._h, 1, 1, ok, 0) == -1 and b'elastic handle' in e._lib.gpf_last_error()
    # surrogate closures
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = quiet(Problem.from_string, SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            g.set_lines([{'along': 'x'}])
        quiet(g._pre_run)
        assert g._lib.gpf_lines_set(g._h, 1, 1, ok, 0) == -1 and b'surrogate' in g._lib.gpf_last_error()
    # an armed member of an ensemble: member and reason named, by the package and by the library
    members = [tp.build(JOURNAL_1D), tp.build(JOURNAL_1D.replace('eps: 0.7', 'eps: 0.5'))]
    members[1].set_lines([{'along': 'x'}])
    with pytest.raises(NotImplementedError, match='member 1: lines are armed'):
        Ensemble(members)
    handles = (C.c_void_p * 2)(*[m._h.value for m in members])
    ens = C.c_void_p()
    assert members[0]._lib.gpf_ensemble_create(handles, 2, C.byref(ens)) == -1
    assert b'member 1: lines are armed on it (they cut the batch per member; gpf_lines_clear, or step it alone)' in members[0]._lib.gpf_last_error()
    members[1].clear_lines()
    made = Ensemble(members)
    members[0].set_lines([{'along': 'x'}])
    with pytest.raises(NotImplementedError, match='member 0: .*lines are armed'):
        made.step(3)
