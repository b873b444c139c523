"""The step-change series (set_changes / changes / step_change, gpf_changes_*) on the device.

A record compares the committed state with the state before that step, which the device still holds in its other q buffer.  Held
bit for bit: the maxima, their cells and dt against NumPy on the planes downloaded after every step, every stride against
every = 1, one stepping call against twelve, the series against step_change() after each update(), the 8-byte against the 16-byte
loads, the run's q against the run with nothing armed.  Held to a tolerance: the seven sums against math.fsum of the NumPy terms.

Shapes: tests/test_gpu_elastic_series.py's fixed-form Bayada / piezo parabolic slider without the elastic line (V != 0: all three
fields move) on 48 x 30, 48 x 31 (the last pair of a row reaches the ghost column), 260 x 6 (a fold thread adds two rows),
6 x 600 (a thread walks two pairs of its row) and 48 x 30 with D / N edges; the reference suite's 1-D journal bearing, 100 x 1,
which steps through the one-workgroup kernel with its batch cut at every recorded step."""
import contextlib
import ctypes as C
import functools
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import reference_suite as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEP = 12
SUMS = ('d2_rho', 'd2_jx', 'd2_jy', 'q2_rho', 'q2_jx', 'q2_jy', 'dmass')
MAXIMA = ('dmax_rho', 'dmax_jx', 'dmax_jy')
NAMES = SUMS + MAXIMA + ('dt',)

BASE = """
options: {{silent: True{options}}}
grid: {{{grid}}}
geometry: {{type: parabolic, hmin: 2.54e-5, hmax: 5.08e-5, U: 4.57, V: 0.3}}
numerics: {{adaptive: 1, CFL: 0.45, tol: 1e-8, dt: 1.e-10, max_it: 60}}
properties:
    EOS: Bayada
    rho0: 850.
    shear: 0.039
    bulk: 0.
    cl: 1600.
    cv: 352.
{extra}    piezo: {{name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}}
"""
DN = "xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 850., xW_D: 850., yS: ['D', 'N', 'N'], yN: ['D', 'N', 'N'], yS_D: 850., yN_D: 850."
GRIDS = {
    '48x30': "Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 30",
    '48x31': "Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 31",
    '260x6': "Lx: 0.0762, Ly: 0.04, Nx: 260, Ny: 6",
    '6x600': "Lx: 0.009525, Ly: 0.8, Nx: 6, Ny: 600",           # the cells of 48x30
    'dn-48x30': f"Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 30, {DN}",
}
SHAPES = sorted(GRIDS)
ELASTIC = "    elastic: {E: 50e09, v: 0.3, alpha_underrelax: 0.05}\n"
THINNING = "    thinning: {name: Eyring, tauE: 5.e5}\n"
JOURNAL_1D = rs.JOURNAL_1D
FLAT = """
options: {silent: True}
grid: {dx: 1.e-5, dy: 1.e-5, Nx: 48, Ny: 31, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: inclined, hmin: 5.e-6, hmax: 5.e-6, U: 0., V: 0.}
numerics: {CFL: 0.5, adaptive: 1, tol: 1e-8, dt: 1e-10, max_it: 1000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}
"""


def text_of(name, extra='', options=''):
    return BASE.format(grid=GRIDS[name], extra=extra, options=options)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(text):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, text)
    p._pre_run()
    return p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bitwise(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    same = bits(a) == bits(b)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ, max |difference| {np.nanmax(np.abs(a - b)):.3e}"


def series_of(p):
    """(steps, values (n, 11), cells (n, 3, 2), times) of p.changes."""
    s = p.changes
    return s.step.tolist(), np.array([getattr(s, n) for n in NAMES]).T.reshape(len(s.step), len(NAMES)), s.cells.copy(), s.time.copy()


def now_of(p):
    """(values (11,), cells (3, 2)) of p.step_change()."""
    r = p.step_change()
    return np.array([r[n] for n in NAMES]), np.array([r[n + '_cell'] for n in MAXIMA])


def batch_run(text, nstep, every):
    """Armed at `every`, all steps in one stepping call."""
    p = build(text)
    p.set_changes(every)
    p._advance(nstep, honor_stop=False)
    steps, vals, cells, times = series_of(p)
    return dict(steps=steps, vals=vals, cells=cells, times=times, q=p.q.copy())


def stepwise_run(text, nstep, arm):
    """One update() at a time.  Unarmed: q downloaded after each, with the step size the step took.  Armed at every = 1: the series
    and step_change() behind every update."""
    p = build(text)
    if arm:
        p.set_changes(1)
    qs, dts, now, now_cells = [p.q.copy()], [], [], []
    for _ in range(nstep):
        dts.append(p.dt)
        p.update()
        if arm:
            v, c = now_of(p)
            now.append(v)
            now_cells.append(c)
        else:
            qs.append(p.q.copy())
    out = dict(q=p.q.copy(), qs=qs, dts=dts, h=np.array(p.topo.h), dA=p.grid['dx'] * p.grid['dy'])
    if arm:
        steps, vals, cells, times = series_of(p)
        out.update(steps=steps, vals=vals, cells=cells, times=times, now=np.array(now), now_cells=np.array(now_cells))
    return out


@functools.lru_cache(maxsize=None)
def runs(name):
    """Per shape, computed once and only read: A unarmed update by update, B every = 1 in one call, `three` every = 3 in one
    call, `calls` every = 1 update by update with step_change() behind each."""
    text = text_of(name)
    return dict(A=stepwise_run(text, NSTEP, False), B=batch_run(text, NSTEP, 1), three=batch_run(text, NSTEP, 3),
                calls=stepwise_run(text, NSTEP, True))


def numpy_record(qn, qo, h, dA):
    """name -> (fsum of the terms times dx dy, sum |term| dx dy) for the sums; name -> (max |d|, its cell) for the maxima."""
    out = {}
    d = (qn - qo)[:, 1:-1, 1:-1]
    qi, hi = qn[:, 1:-1, 1:-1], h[1:-1, 1:-1]
    terms = {f'd2_{f}': d[k] * d[k] for k, f in enumerate(('rho', 'jx', 'jy'))}
    terms.update({f'q2_{f}': qi[k] * qi[k] for k, f in enumerate(('rho', 'jx', 'jy'))})
    terms['dmass'] = d[0] * hi
    for n, t in terms.items():
        out[n] = (math.fsum(t.ravel().tolist()) * dA, math.fsum(np.abs(t).ravel().tolist()) * dA)
    for k, n in enumerate(MAXIMA):
        a = np.abs(d[k])
        ix, iy = divmod(int(np.argmax(a)), a.shape[1])
        out[n] = (a[ix, iy], (ix + 1, iy + 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (a) against NumPy
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SHAPES)
def test_values_match_numpy_on_the_downloaded_planes(hiplib, name):
    """Every record of the one-call run against NumPy on the planes the unarmed run downloaded after every update(): the maxima,
    their cells (np.argmax over the C-ordered interior is the record's tie rule) and dt in every bit, the sums within
    64 * 2^-53 * sum|term| dx dy of math.fsum of the terms.  The bound: a tree less than 24 additions deep on these shapes, one
    rounding per difference, one per product and one for dx dy.  Each figure is printed as error / bound before it is asserted.
    Both runs end on the same q in every bit: recording only reads."""
    r = runs(name)
    A, B = r['A'], r['B']
    assert B['steps'] == list(range(1, NSTEP + 1)) and B['cells'].shape == (NSTEP, 3, 2) and B['cells'].dtype == np.int32
    u = 2.0 ** -53
    worst, exact = {n: 0. for n in SUMS}, []
    for k in range(NSTEP):
        ref = numpy_record(A['qs'][k + 1], A['qs'][k], A['h'], A['dA'])
        got = dict(zip(NAMES, B['vals'][k]))
        for n in SUMS:
            val, mag = ref[n]
            w = abs(got[n] - val) / (64. * u * mag) if mag > 0 else (0. if got[n] == val else np.inf)
            worst[n] = max(worst[n], w)
        for j, n in enumerate(MAXIMA):
            if not (bits(got[n]) == bits(ref[n][0]) and tuple(B['cells'][k, j]) == ref[n][1]):
                exact.append((k + 1, n, got[n], tuple(B['cells'][k, j]), ref[n]))
        if not bits(got['dt']) == bits(A['dts'][k]):
            exact.append((k + 1, 'dt', got['dt'], A['dts'][k]))
    print(f"\n[{name}] worst |device - fsum| / (64 u sum|term|) over {NSTEP} steps: " + ', '.join(f"{n} {w:.3e}" for n, w in worst.items()))
    assert not exact, f"{name}: (step, name, device, ...) not bitwise NumPy's: {exact[:4]}"
    bad = {n: w for n, w in worst.items() if not w <= 1.0}
    assert not bad, f"{name}: outside the bound (error / bound): {bad}"
    assert_bitwise(B['q'], A['q'], f"{name}: q of the armed run against q of the unarmed run")


# ---------------------------------------------------------------------------------------------------------------------------
# (b) bitwise invariances
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SHAPES)
def test_records_do_not_depend_on_stride_or_batching(hiplib, name):
    r = runs(name)
    B, three, calls = r['B'], r['three'], r['calls']
    assert three['steps'] == [3, 6, 9, 12]
    assert_bitwise(three['vals'], B['vals'][2::3], f"{name}: every = 3 against every = 1")
    assert three['cells'].tolist() == B['cells'][2::3].tolist()
    assert_bitwise(three['times'], B['times'][2::3], f"{name}: times")
    assert calls['steps'] == B['steps']
    assert_bitwise(calls['vals'], B['vals'], f"{name}: twelve update() calls against one stepping call")
    assert calls['cells'].tolist() == B['cells'].tolist()
    assert_bitwise(calls['vals'], calls['now'], f"{name}: the series against step_change() after each update")
    assert calls['cells'].tolist() == calls['now_cells'].tolist()
    for x in (three, calls):
        assert_bitwise(x['q'], r['A']['q'], f"{name}: q with changes armed against q with nothing armed")


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_changes as t
out = {{}}
for name in t.SHAPES:
    b = t.batch_run(t.text_of(name), t.NSTEP, 1)
    out[name + '_vals'], out[name + '_cells'] = b['vals'], b['cells']
np.savez({out!r}, **out)
"""


def test_narrow_loads_give_the_same_bits(hiplib, tmp_path):
    """GPF_FILM_NARROW is read when the buffers are allocated: a fresh child process records every shape with the 8-byte loads --
    that it did take them is read from the library's GPF_DEBUG trace of the allocation -- and leaves the bits of this process,
    which took the 16-byte loads."""
    out = str(tmp_path / 'narrow.npz')
    cmd = [sys.executable, '-c', CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)]
    res = subprocess.run(cmd, env=dict(os.environ, GPF_DEBUG='1', GPF_FILM_NARROW='1'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr.count('k_change_partial takes 8-byte pair loads') == len(SHAPES) and 'k_change_partial takes 16-byte' not in res.stderr
    narrow = np.load(out)
    for name in SHAPES:
        wide = runs(name)['B']
        assert_bitwise(narrow[name + '_vals'], wide['vals'], f"{name}: narrow against wide loads")
        assert narrow[name + '_cells'].tolist() == wide['cells'].tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the one-workgroup kernel: the batch is cut at every recorded step
# ---------------------------------------------------------------------------------------------------------------------------
def test_small_grid_batches_are_cut_at_the_recorded_steps(hiplib):
    n = 40
    calls = stepwise_run(JOURNAL_1D, n, True)
    plain = build(JOURNAL_1D)
    plain._advance(n, honor_stop=False)
    assert calls['steps'] == list(range(1, n + 1))
    assert_bitwise(calls['vals'], calls['now'], 'update by update: the series against step_change()')
    assert float(calls['vals'][:, NAMES.index('dmax_rho')].max()) > 0.       # the bearing does move
    for every in (1, 7):
        b = batch_run(JOURNAL_1D, n, every)
        assert b['steps'] == list(range(every, n + 1, every))
        pick = [s - 1 for s in b['steps']]
        assert_bitwise(b['vals'], calls['now'][pick], f"100x1, every = {every}: one call against step_change() after each update")
        assert b['cells'].tolist() == calls['now_cells'][pick].tolist()
        assert_bitwise(b['q'], plain.q, f"100x1, every = {every}: q against the unarmed run's")
    assert_bitwise(calls['q'], plain.q, '100x1, update by update: q against the unarmed run')


# ---------------------------------------------------------------------------------------------------------------------------
# (d) a field at rest
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_field_at_rest_records_zeros(hiplib):
    """A flat gap, U = V = 0 and the uniform initial state: where a field did not move, its d2 and dmax are +0.0 and its cell is
    (1, 1), the first under the tie rule.  Which fields rest in which step is read from the planes an unarmed run downloads after
    every update(): rho and jy rest in all three steps; the solver's first step moves jx off the uploaded state by about 1e-17 per
    cell (measured: d2_jx = 9.7e-41 in step 1) before it rests too, and there the record must be NumPy's in every bit instead.
    That pattern is pinned: (step 1, jx) moves and the other eight pairs rest, so that no further pair can begin to move unseen."""
    A = stepwise_run(FLAT, 3, False)
    B = batch_run(FLAT, 3, 1)
    assert B['steps'] == [1, 2, 3]
    assert_bitwise(B['q'], A['q'], 'q of the armed run against the unarmed run')
    moved = []
    for k in range(3):
        got = dict(zip(NAMES, B['vals'][k]))
        ref = numpy_record(A['qs'][k + 1], A['qs'][k], A['h'], A['dA'])
        for j, f in enumerate(('rho', 'jx', 'jy')):
            if np.array_equal(bits(A['qs'][k + 1][j, 1:-1, 1:-1]), bits(A['qs'][k][j, 1:-1, 1:-1])):
                assert bits(got[f'd2_{f}']) == bits(0.0) and bits(got[f'dmax_{f}']) == bits(0.0), (k + 1, f, got)
                assert tuple(B['cells'][k, j]) == (1, 1), (k + 1, f, B['cells'][k, j])
                if f == 'rho':
                    assert bits(got['dmass']) == bits(0.0), (k + 1, got['dmass'])
            else:
                moved.append((k + 1, f))
                assert bits(got[f'dmax_{f}']) == bits(ref[f'dmax_{f}'][0]) and tuple(B['cells'][k, j]) == ref[f'dmax_{f}'][1], (k + 1, f)
    assert moved == [(1, 'jx')], f"the (step, field) pairs that are not at rest: {moved}"
    assert (B['vals'][:, NAMES.index('q2_rho')] > 0).all() and (B['vals'][:, NAMES.index('dt')] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) a rolled-back step leaves no record
# ---------------------------------------------------------------------------------------------------------------------------
def test_rolled_back_step_leaves_no_record(hiplib):
    """tests/test_gpu_parity.py: test_invalid_state_rolls_back's way to an invalid state (an absurd time step): the scalar log keeps
    its entry for the invalid step, the series ends one entry before it, and step_change() refuses the flagged state."""
    from gapflow_amd import _lib
    p = build(text_of('48x30'))
    p.set_changes(1)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_changes_read(p._h, None, None, 0, None, C.byref(have)))
    assert have.value == 0
    np.testing.assert_array_equal(p.q, good)
    steps, vals, cells, _ = series_of(p)
    assert steps == [1, 2, 3]
    assert_bitwise(vals, runs('48x30')['B']['vals'][:3], 'records before the rollback')
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.step_change()


# ---------------------------------------------------------------------------------------------------------------------------
# (f) step_change() needs the state before the last step on the device
# ---------------------------------------------------------------------------------------------------------------------------
def test_step_change_names_why_the_previous_state_is_gone(hiplib):
    from gapflow_amd import _lib
    p = build(text_of('48x30'))
    with pytest.raises(_lib.GapflowHipError, match='no step has been committed since'):
        p.step_change()                                 # before any step
    p.update()
    first = now_of(p)
    assert_bitwise(first[0], runs('48x30')['B']['vals'][0], 'step_change() after the first update')
    p.q[0, 5, 5] *= 1.0 + 2.0 ** -40                    # the host's edit is uploaded: the other buffer is no neighbour of this state
    with pytest.raises(_lib.GapflowHipError, match='no step has been committed since'):
        p.step_change()
    p.update()
    assert p.step_change()['dmax_rho'] > 0.
    coarse = build(text_of('48x30').replace('Nx: 48, Ny: 30', 'Nx: 24, Ny: 15'))
    coarse.update()
    quiet(p.init_from, coarse)
    with pytest.raises(_lib.GapflowHipError, match='no step has been committed since'):
        p.step_change()
    p.update()
    assert p.step_change()['dmax_rho'] > 0.
    p.pressure.pressure                                 # redoes the predictor of the last step into the other buffer
    with pytest.raises(_lib.GapflowHipError, match='gpf_update_closures has reused the buffer'):
        p.step_change()
    p.update()
    rec = p.step_change()
    assert rec['dmax_rho'] > 0. and rec['dt'] > 0.
    # stage-wise steps on the same handle
    lib = p._lib
    _lib.check(lib.gpf_open_step(p._h))
    vals, cells = np.zeros(11), np.zeros(6, dtype=np.int32)
    vp, cp = vals.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.gpf_changes_now(p._h, vp, cp) == -5 and b'open' in lib.gpf_last_error()
    assert lib.gpf_changes_set(p._h, 1) == -5 and b'open' in lib.gpf_last_error()
    for stage in range(2):
        _lib.check(lib.gpf_stage_closures(p._h))
        _lib.check(lib.gpf_stage_advance(p._h, stage))
    _lib.check(lib.gpf_close_step(p._h, None))
    assert lib.gpf_changes_now(p._h, vp, cp) == -5 and b'the last step was stage-wise' in lib.gpf_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# (g) refusals and lifecycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(hiplib):
    from gapflow_amd import _lib
    vals, cells = np.zeros(11), np.zeros(6, dtype=np.int32)
    vp, cp = vals.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_int32))
    ms = C.c_double(0.)
    for extra, word in ((THINNING, b'shear thinning'), (ELASTIC, b'elastic')):
        p = build(text_of('48x30', extra=extra))
        lib = p._lib
        with pytest.raises(NotImplementedError, match='step stage-wise'):
            p.set_changes(1)
        with pytest.raises(NotImplementedError, match='step stage-wise'):
            p.step_change()
        assert p.changes is None
        assert lib.gpf_changes_set(p._h, 1) == -1 and word in lib.gpf_last_error()
        assert lib.gpf_changes_now(p._h, vp, cp) == -1 and word in lib.gpf_last_error()
        assert lib.gpf_changes_time(p._h, 1, 0, C.byref(ms)) == -1 and word in lib.gpf_last_error()
        with pytest.raises(NotImplementedError, match='step stage-wise'):
            build(text_of('48x30', extra=extra, options=', changes: 2'))
    rigid = build(text_of('48x30'))
    lib = rigid._lib
    with pytest.raises(ValueError, match='changes: the stride must be an integer >= 1'):
        rigid.set_changes(0)
    assert lib.gpf_changes_set(rigid._h, 0) == -1 and b'every >= 1' in lib.gpf_last_error()
    assert lib.gpf_changes_read(rigid._h, None, None, 0, None, None) == -5 and b'no changes are armed' in lib.gpf_last_error()
    assert lib.gpf_changes_time(rigid._h, 1, 1, C.byref(ms)) == -5 and b'mode 1 needs armed changes' in lib.gpf_last_error()
    assert lib.gpf_changes_set(None, 1) == -1
    # a slab handle: halo rows on one side
    cfg = rigid._make_config(0)
    cfg.halo_lo = 1
    slab = C.c_void_p()
    _lib.check(lib.gpf_create(C.byref(cfg), C.byref(slab)))
    try:
        assert lib.gpf_changes_set(slab, 1) == -5 and b'slab' in lib.gpf_last_error()
    finally:
        lib.gpf_destroy(slab)
    # an armed member of an ensemble: member and reason named, by the package and by the library
    from gapflow_amd import Ensemble
    members = [build(JOURNAL_1D), build(JOURNAL_1D)]
    members[1].set_changes(1)
    with pytest.raises(NotImplementedError, match=r'member 1: changes are armed on it \(they cut the batch per member\): clear_changes\(\)'):
        Ensemble(members)
    handles = (C.c_void_p * 2)(*[m._h.value for m in members])
    ens = C.c_void_p()
    assert lib.gpf_ensemble_create(handles, 2, C.byref(ens)) == -1
    assert b'member 1: changes are armed on it (they cut the batch per member; gpf_changes_clear, or step it alone)' in lib.gpf_last_error()
    members[1].clear_changes()
    Ensemble(members)


def test_surrogate_closures_are_refused(hiplib):
    """tests/test_gpu_probes.py: SURROGATE (pressure and shear from Gaussian processes; the handle holds its models after
    _pre_run): by the package before any library call, by the library in all three calls that would record."""
    import warnings
    from gapflow_amd import Problem
    import test_gpu_probes as tp
    vals, cells = np.zeros(11), np.zeros(6, dtype=np.int32)
    vp, cp = vals.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_int32))
    ms = C.c_double(0.)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p = quiet(Problem.from_string, tp.SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            p.set_changes(1)
        with pytest.raises(NotImplementedError, match='surrogate'):
            p.step_change()
        with pytest.raises(NotImplementedError, match='surrogate'):
            quiet(Problem.from_string, tp.SURROGATE.replace('write_freq: 100}', 'write_freq: 100, changes: 2}'))
        quiet(p._pre_run)
        lib = p._lib
        assert lib.gpf_changes_set(p._h, 1) == -1 and b'surrogate' in lib.gpf_last_error()
        assert lib.gpf_changes_now(p._h, vp, cp) == -1 and b'surrogate' in lib.gpf_last_error()
        assert lib.gpf_changes_time(p._h, 1, 0, C.byref(ms)) == -1 and b'surrogate' in lib.gpf_last_error()
    assert p.changes is None


# ---------------------------------------------------------------------------------------------------------------------------
# gpf_changes_time, and changes inside the other series' gpf_*_time calls (tests/test_gpu_series_time.py's rule and its twins)
# ---------------------------------------------------------------------------------------------------------------------------
def changes_records(p):
    """(number of records, their step counts, values, cells) of the last stepping call, zero-padded."""
    import test_gpu_series_time as ts
    from gapflow_amd import _lib
    n, steps = C.c_int64(-1), np.zeros(ts.CAP, dtype=np.int64)
    vals, cells = np.zeros((ts.CAP, 11)), np.zeros((ts.CAP, 6), dtype=np.int32)
    ts.ok(p, p._lib.gpf_changes_read(p._h, _lib.as_dp(vals), cells.ctypes.data_as(ts.I32P), ts.CAP, steps.ctypes.data_as(ts.I64P), C.byref(n)))
    return n.value, steps, vals, cells


def same_changes(ra, rb):
    return ra[0] == rb[0] and (ra[1] == rb[1]).all() and bool((bits(ra[2]) == bits(rb[2])).all()) and (ra[3] == rb[3]).all()


def armed_with_all(text):
    """test_gpu_series_time's problem, its seven series armed and WARM steps in, and changes at every = 3 beside them."""
    import test_gpu_series_time as ts
    p = ts.armed(text)
    p.set_changes(3)
    return p


@pytest.mark.parametrize('grid', ['small-1d', 'step2-37x71'])
@pytest.mark.parametrize('mode', [0, 1])
def test_changes_time_steps_and_records_as_gpf_step_does(hiplib, grid, mode):
    """A takes TIMED steps through gpf_changes_time, its twin B through gpf_step, then both AFTER more through gpf_step: the same
    state; mode 1 leaves gpf_step's records of the changes, mode 0 none; no other series keeps a record of the call; the
    statistics window restarts; afterwards every series, changes included, records as the twin's: all were armed again."""
    import test_gpu_series_time as ts
    a, b = armed_with_all(ts.GRIDS[grid]), armed_with_all(ts.GRIDS[grid])
    f = ts.Findings()
    ms = ts.timed(a, 'changes', ts.TIMED, mode)
    ts.step(b, ts.TIMED)
    f.expect(np.isfinite(ms) and ms > 0, f"ms = {ms}")
    f.expect(ts.step_count(a) == ts.step_count(b) == ts.WARM + ts.TIMED, f"step counts {ts.step_count(a)} and {ts.step_count(b)}")
    f.expect(ts.same_bits(ts.state(a), ts.state(b)), "the states differ after the timed steps")
    ra, rb = changes_records(a), changes_records(b)
    f.expect(rb[0] == 4 and rb[1][:4].tolist() == [6, 9, 12, 15], f"the gpf_step twin's changes: {rb[0]} records at {rb[1][:rb[0]].tolist()}")
    if mode == 1:
        f.expect(same_changes(ra, rb), f"the timed changes differ from gpf_step's ({ra[0]} records at {ra[1][:ra[0]].tolist()})")
    else:
        f.expect(ra[0] == 0, f"changes report {ra[0]} records after mode 0")
    for s in ts.SERIES[:6]:
        f.expect(ts.records(a, s)[0] == 0, f"{s} report {ts.records(a, s)[0]} records after gpf_changes_time")
    f.expect(ts.window(a)[0] == 0, f"the statistics window was not restarted: {ts.window(a)}")
    ts.expect_same_run_after(f, a, b, f"after mode {mode}")
    ra, rb = changes_records(a), changes_records(b)
    f.expect(rb[0] == 2 and same_changes(ra, rb), f"changes after the next call: {ra[0]} records at {ra[1][:ra[0]].tolist()}, the twin's {rb[0]}")
    f.settle()


@pytest.mark.parametrize('grid', ['small-1d', 'step2-37x71'])
@pytest.mark.parametrize('series', ['integrals', 'extrema'])
def test_another_series_time_call_puts_changes_aside_and_brings_them_back(hiplib, grid, series):
    import test_gpu_series_time as ts
    a, b = armed_with_all(ts.GRIDS[grid]), armed_with_all(ts.GRIDS[grid])
    ts.step(a, 3)
    ts.step(b, 3)
    assert changes_records(a)[0] == 1                   # a record from before the call, which must not survive it
    f = ts.Findings()
    ts.timed(a, series, ts.TIMED - 3, 1)
    ts.step(b, ts.TIMED - 3)
    f.expect(ts.same_bits(ts.state(a), ts.state(b)), "the states differ after the timed steps")
    f.expect(changes_records(a)[0] == 0, f"changes report {changes_records(a)[0]} records after gpf_{series}_time")
    f.expect(ts.same_records(ts.records(a, series), ts.records(b, series)), f"the timed {series} differ from gpf_step's")
    ts.expect_same_run_after(f, a, b, f"after gpf_{series}_time")
    ra, rb = changes_records(a), changes_records(b)
    f.expect(rb[0] == 2 and same_changes(ra, rb), f"changes after the next call: {ra[0]} records at {ra[1][:ra[0]].tolist()}, the twin's {rb[0]}")
    f.settle()


def test_clear_and_rearm_start_a_new_series(hiplib):
    p = build(text_of('48x30'))
    p.set_changes(1)
    p._advance(3, honor_stop=False)
    assert p.changes.step.tolist() == [1, 2, 3]
    p.clear_changes()
    assert p.changes is None
    p._advance(1, honor_stop=False)
    p.set_changes(2)
    assert p.changes.step.shape == (0,) and p.changes.cells.shape == (0, 3, 2) and p.changes.cells.dtype == np.int32
    p._advance(4, honor_stop=False)
    steps, vals, cells, _ = series_of(p)
    assert steps == [6, 8]
    B = runs('48x30')['B']
    assert_bitwise(vals, B['vals'][[5, 7]], 're-armed at every = 2 against every = 1')
    assert cells.tolist() == B['cells'][[5, 7]].tolist()
    p._pre_run()
    assert p.changes.step.shape == (0,)


def flatten(x, prefix=''):
    """Every array of a series (namedtuple, dict, nested) as (name, array)."""
    if x is None:
        return []
    if hasattr(x, '_asdict'):
        x = x._asdict()
    if isinstance(x, dict):
        return [item for k, v in x.items() for item in flatten(v, f'{prefix}{k}.')]
    try:
        a = np.asarray(x)
    except (TypeError, ValueError):
        return []
    return [(prefix[:-1], a)] if a.dtype.kind in 'fiu' else []


def test_the_other_series_record_the_same_beside_changes(hiplib):
    """All other series a rigid problem accepts, armed with and without changes: their records agree in every bit, and the
    changes' own equal those taken alone."""
    def run(with_changes):
        p = build(text_of('48x30'))
        nx, ny = p.grid['Nx'], p.grid['Ny']
        p.set_probes([[1, 1], [24, 15], [48, 30]], pressure=True)
        p.set_integrals(2)
        p.set_weighted_integrals(np.ones((nx, ny)), 3)
        p.set_regions([{'field': 'rho', 'below': 850.0, 'name': 'low'}], 2)
        p.set_lines([{'along': 'x'}, {'along': 'y', 'at': [1, 10], 'name': 'band'}], 3)
        p.set_extrema(1)
        p.set_statistics(2)
        if with_changes:
            p.set_changes(1)
        p._advance(NSTEP, honor_stop=False)
        out = []
        for name in ('probes', 'integrals', 'weighted_integrals', 'regions', 'lines', 'extrema', 'statistics'):
            out += flatten(getattr(p, name), name + '.')
        return out, p
    with_, p = run(True)
    without, _ = run(False)
    assert [n for n, _ in with_] == [n for n, _ in without] and len(with_) > 40
    for (n, a), (_, b) in zip(with_, without):
        if a.dtype.kind == 'f':
            assert_bitwise(a, b, n)
        else:
            assert a.tolist() == b.tolist(), n
    steps, vals, cells, _ = series_of(p)
    B = runs('48x30')['B']
    assert steps == B['steps']
    assert_bitwise(vals, B['vals'], 'changes beside every other series against changes alone')
    assert cells.tolist() == B['cells'].tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# (h) run() and restore
# ---------------------------------------------------------------------------------------------------------------------------
def run_yaml(out, silent, max_it=12):
    return text_of('48x30', options=f", output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, changes: 2") \
        .replace('options: {silent: True, ', 'options: {').replace('max_it: 60', f'max_it: {max_it}')


def test_run_writes_changes_npz_and_a_restored_problem_rearms(hiplib, tmp_path):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'changes.npz'))
    assert sorted(f.files) == sorted(['step', 'time', 'names', 'cells'] + list(NAMES))
    assert f['names'].tolist() == list(MAXIMA) and f['step'].tolist() == [2, 4, 6, 8, 10, 12] and f['cells'].shape == (6, 3, 2)
    B = runs('48x30')['B']
    for k, n in enumerate(NAMES):
        assert_bitwise(f[n], B['vals'][1::2, k], f"run() at stride 2 against the batch at stride 1: {n}")
    assert f['cells'].tolist() == B['cells'][1::2].tolist()
    # checkpoints do not carry the series: the restored problem re-arms from its options and records from the restart step
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(7, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.changes.step.shape == (0,) and b.changes.cells.shape == (0, 3, 2)
    assert_bitwise(now_of(b)[0], B['vals'][4], 'step_change() of the restored state: the checkpoint carries the previous state')
    b._advance(7, honor_stop=False)
    assert a.changes.step.tolist() == [2, 4, 6, 8, 10, 12] and b.changes.step.tolist() == [6, 8, 10, 12]
    assert_bitwise(series_of(b)[1], series_of(a)[1][2:], 'continued against restored')
    assert series_of(b)[2].tolist() == series_of(a)[2][2:].tolist()
