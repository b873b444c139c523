"""Point probes (gpf_probes_*, Problem.set_probes / probes, options.probes): per-step time series at chosen cells, recorded on
the device while gpf_step advances whole batches.

The yardstick throughout is a second, identical Problem advanced by update() one step at a time with .q read after every step
(the path the goldens pin): the probed batch's rho / jx / jy equal the twin's q at those cells after each step in every bit, its
`time` equals the twin's simtime, and the run itself -- final q, every scalar -- equals, in every bit, the same batch without
probes: recording only reads.  p is held to models.pressure.eos_pressure of the recorded density at rtol 1e-12, the tolerance
test_eos_pressure_and_sound_speed holds the device EOS to.  Reference: none (the reference reads q on the host after every step)."""
import contextlib
import functools
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ('step', 'simtime', 'dt', 'ekin', 'ekin_old', 'residual', 'v_max', 'v_sound', 'mass', 'invalid', 'converged')
DN = "xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']"

# the 1-D journal bearing of the README's small-grid figure (one workgroup: k_small_steps)
JOURNAL_1D = """
options: {silent: True}
grid: {dx: 1.e-5, dy: 1., Nx: 100, Ny: 1, %s, xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325, rho0: 877.7007, C1: 3.5e10, C2: 1.23}
""" % DN
# a law that goes through pow(), on the same grid
INCLINED_PL = """
options: {silent: True}
grid: {Lx: 0.1, Ly: 1., Nx: 100, Ny: 1, %s, xE_D: 1.1853, xW_D: 1.1853}
geometry: {type: inclined, hmax: 6.6e-5, hmin: 1e-5, U: 50., V: 0.}
numerics: {CFL: 0.4, adaptive: True, tol: 1e-12, dt: 1e-8, max_it: 100000}
properties: {EOS: PL, shear: 1.846e-5, bulk: 0., P0: 101325, rho0: 1.1853, alpha: 0.}
""" % DN
CELLS_1D = [(0, 1), (1, 1), (50, 1), (100, 1), (101, 1), (50, 0), (50, 2)]

# 128 x 130: off the small-grid kernel; Ny = 130 is one full 126-column strip and a ragged one
TWO_D = """
options: {{silent: True}}
grid: {{Nx: 128, Ny: 130, Lx: 0.02, Ly: 0.03, {bc}}}
geometry: {geo}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1e-14, dt: 2.e-9, max_it: 100000}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}}
"""
# x-only gap: k_step2 reads the row-coefficient table; MC_order 0: parity and sweep direction alternate
SLIDER_2D = TWO_D.format(bc=DN + ", xE_D: 877.7007, xW_D: 877.7007", geo="{type: inclined, hmax: 1.2e-5, hmin: 4.e-6, U: 0.5, V: 0.}")
# gap planes, all periodic
ASPERITY_2D = TWO_D.format(bc="xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']",
                           geo="{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.05}")
# the four corners, both ghost rows, both ghost columns, columns 126 / 127 / 128 (the seam between two wavefronts' strips)
CELLS_2D = [(0, 0), (0, 131), (129, 0), (129, 131), (0, 60), (129, 60), (64, 0), (64, 131), (64, 126), (64, 127), (64, 128),
            (1, 1), (128, 130), (37, 1)]

# tests/test_gpu_checkpoint.py: THINNING (Eyring, 48 x 10; stage-wise steps), restated
THINNING = """
options: {silent: True}
grid: {Nx: 48, Ny: 10, Lx: 0.05, Ly: 0.01, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: parabolic, hmin: 1.e-5, hmax: 4.e-5, U: 10., V: 1.}
numerics: {CFL: 0.4, adaptive: 1, max_it: 100}
properties:
    EOS: DH
    shear: 0.05
    bulk: 0.
    rho0: 877.7007
    thinning: {name: Eyring, tauE: 5.e5}
"""

CASES = {'small-1d': (JOURNAL_1D, CELLS_1D, 50), 'slider-rowcoef': (SLIDER_2D, CELLS_2D, 12), 'asperity-planes': (ASPERITY_2D, CELLS_2D, 8),
         'power-law-1d': (INCLINED_PL, CELLS_1D, 20)}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(text):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, text)
    p._pre_run()
    return p


def scalars_of(p):
    sc = p._scalars()
    return tuple(getattr(sc, k) for k in SCALARS)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bitwise(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    same = bits(a) == bits(b)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ, max |difference| {np.nanmax(np.abs(a - b)):.3e}"


def stepped(p, cells, n):
    """n single update() calls with q read after each: (step, time, values (n, ncells, 3)) at the cells."""
    ix, iy = np.array(cells).T
    step, time, val = [], [], []
    for _ in range(n):
        p.update()
        step.append(p.step)
        time.append(p.simtime)
        val.append(p.q[:, ix, iy].T.copy())
    return np.array(step), np.array(time), np.array(val)


def assert_series_is(series, twin, what):
    step, time, val = twin
    assert series.step.tolist() == step.tolist(), what
    assert_bitwise(series.time, time, f"{what}: time")
    for c, name in enumerate(('rho', 'jx', 'jy')):
        assert_bitwise(getattr(series, name), val[:, :, c], f"{what}: {name}")


@functools.lru_cache(maxsize=None)
def case_runs(name):
    """One probed batch, the stepped twin and the same batch without probes; computed once per case and only read by the tests."""
    text, cells, n = CASES[name]
    probed, twin, plain = build(text), build(text), build(text)
    probed.set_probes(cells, pressure=True)
    log = probed._advance(n, honor_stop=False)
    plain_log = plain._advance(n, honor_stop=False)
    return dict(series=probed.probes, twin=stepped(twin, cells, n), q=probed.q.copy(), scalars=scalars_of(probed),
                log=[tuple(getattr(e, k) for k in SCALARS) for e in log], plain_q=plain.q.copy(), plain_scalars=scalars_of(plain),
                plain_log=[tuple(getattr(e, k) for k in SCALARS) for e in plain_log], twin_q=twin.q.copy(), prop=probed.prop)


def assert_same_scalars(a, b, what):
    for k, x, y in zip(SCALARS, a, b):
        if isinstance(x, float):
            assert bits(x) == bits(y), f"{what}: {k} {x!r} vs {y!r}"
        else:
            assert x == y, f"{what}: {k} {x!r} vs {y!r}"


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef', 'asperity-planes'])
def test_batch_series_is_the_stepped_twins_q(hiplib, name):
    """The three places a fused step is recorded from: k_small_steps; k_step2 on an x-only gap (row-coefficient table, alternating sweeps); k_step2 on gap
    planes, all periodic."""
    _, cells, n = CASES[name]
    r = case_runs(name)
    s = r['series']
    assert s.cells.tolist() == [list(c) for c in cells]
    assert s.step.tolist() == list(range(1, n + 1)) and s.rho.shape == (n, len(cells)) and s.p.shape == (n, len(cells))
    assert_series_is(s, r['twin'], name)
    assert_bitwise(r['q'], r['twin_q'], 'final q against the stepped twin')


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef', 'asperity-planes'])
def test_recording_leaves_the_run_unchanged(hiplib, name):
    r = case_runs(name)
    assert_bitwise(r['q'], r['plain_q'], 'final q with and without probes')
    assert_same_scalars(r['scalars'], r['plain_scalars'], 'final scalars')
    assert len(r['log']) == len(r['plain_log'])
    for i, (a, b) in enumerate(zip(r['log'], r['plain_log'])):
        assert_same_scalars(a, b, f"scalar record of step {i + 1}")


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef', 'asperity-planes', 'power-law-1d'])
def test_pressure_is_the_eos_of_the_recorded_density(hiplib, name):
    from gapflow_amd.models.pressure import eos_pressure
    r = case_runs(name)
    s = r['series']
    assert np.all(np.isfinite(s.p)) and np.ptp(s.rho) > 0
    np.testing.assert_allclose(s.p, eos_pressure(s.rho, r['prop']), rtol=1e-12, atol=0.)
    if name == 'power-law-1d':
        assert_series_is(s, r['twin'], name)


CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import test_gpu_probes as t
p = t.build(t.SLIDER_2D)
p.set_probes(t.CELLS_2D, pressure=False)
p._advance(6, honor_stop=False)
s = p.probes
np.savez({out!r}, step=s.step, time=s.time, rho=s.rho, jx=s.jx, jy=s.jy, q=p.q)
"""


def test_split_edge_form_records_the_same_series(hiplib, tmp_path):
    """GPF_STEP_UNFUSED_EDGES=1 is read at gpf_create: a fresh child process runs case 2's problem in the split form (three
    launches per step, the commit in k_ghost_fill); its series equals the fused form's in every bit of rho / jx / jy (the two
    forms sum the kinetic energy in different orders, which the field does not see)."""
    out = str(tmp_path / 'split.npz')
    env = dict(os.environ, GPF_STEP_UNFUSED_EDGES='1')
    res = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    split = np.load(out)
    fused = case_runs('slider-rowcoef')['series']
    assert split['step'].tolist() == list(range(1, 7))
    for name in ('rho', 'jx', 'jy'):
        assert_bitwise(split[name], getattr(fused, name)[:6], f"split against fused: {name}")


def test_max_it_under_honor_stop_ends_the_series(hiplib):
    for text in (JOURNAL_1D, SLIDER_2D):
        p = build(text.replace('max_it: 100000', 'max_it: 7'))
        p.set_probes(CELLS_1D[:3], pressure=False)
        p._advance(20, honor_stop=True)
        s = p.probes
        assert p.step == 7 and s.step.tolist() == list(range(1, 8)) and s.rho.shape == (7, 3) and s.p is None
        ix, iy = np.array(CELLS_1D[:3]).T
        assert_bitwise(s.rho[-1], p.q[0, ix, iy], 'last record against q')


@pytest.mark.parametrize('text', [JOURNAL_1D, SLIDER_2D], ids=['small-1d', 'slider'])
def test_rolled_back_step_leaves_no_record(hiplib, text):
    """tests/test_gpu_parity.py: test_invalid_state_rolls_back's way to an invalid state (an absurd time step): the scalar log
    keeps its entry for the invalid step, the probe series ends at the last valid one, and the problem reports the rollback."""
    p = build(text)
    cells = CELLS_1D[:4]
    ix, iy = np.array(cells).T
    p.set_probes(cells, pressure=True)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    np.testing.assert_array_equal(p.q, good)
    s = p.probes
    assert s.step.tolist() == [1, 2, 3] and s.rho.shape == (3, 4)
    assert_bitwise(s.rho[-1], good[0, ix, iy], 'last record against the state the rollback kept')


@pytest.mark.parametrize('text', [JOURNAL_1D, SLIDER_2D], ids=['small-1d', 'slider'])
def test_nan_in_q_leaves_no_record(hiplib, text):
    """The other flag of an invalid state: a numeric NaN in q (written through the host mirror into a cell that is no probe).
    The step that meets it is rolled back: no record, the series ends at the last valid step, the problem stops."""
    p = build(text)
    cells = CELLS_1D[:4]
    ix, iy = np.array(cells).T
    p.set_probes(cells, pressure=True)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p.q[0, 60, 1] = np.nan
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    s = p.probes
    assert s.step.tolist() == [1, 2, 3] and s.rho.shape == (3, 4) and np.all(np.isfinite(s.p))
    assert_bitwise(s.rho[-1], good[0, ix, iy], 'last record against the last valid state')


def test_stage_wise_steps(hiplib):
    """Eyring thinning takes gpf_open_step ... gpf_close_step: one record per closed step."""
    p, plain = build(THINNING), build(THINNING)
    cells = [(0, 0), (1, 1), (24, 5), (48, 10), (49, 11), (24, 0)]
    p.set_probes(cells, pressure=True)
    twin = stepped(p, cells, 4)
    for _ in range(4):
        plain.update()
    s = p.probes
    assert s.step.tolist() == [1, 2, 3, 4]
    assert_series_is(s, twin, 'thinning')
    assert_bitwise(p.q, plain.q, 'final q with and without probes')
    assert_same_scalars(scalars_of(p), scalars_of(plain), 'final scalars')
    from gapflow_amd.models.pressure import eos_pressure
    np.testing.assert_allclose(s.p, eos_pressure(s.rho, p.prop), rtol=1e-12, atol=0.)


def run_yaml(out, silent, pressure, max_it=12):
    options = f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, probes: [[0, 1], [50, 1], [101, 1]], probes_pressure: {pressure}}}"
    return JOURNAL_1D.replace("options: {silent: True}", options).replace('max_it: 100000', f'max_it: {max_it}')


def test_run_writes_probes_npz_and_a_continuation_appends(hiplib, tmp_path):
    from gapflow_amd import Problem
    out = tmp_path / 'run'
    p = quiet(Problem.from_string, run_yaml(out, False, True))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'probes.npz'))
    assert sorted(f.files) == ['cells', 'jx', 'jy', 'p', 'rho', 'step', 'time']
    assert f['step'].tolist() == list(range(1, 13)) and f['rho'].shape == (12, 3) and f['cells'].tolist() == [[0, 1], [50, 1], [101, 1]]
    hist = dict(zip(p.history['step'], p.history['time']))
    for k in (5, 10):
        assert bits(f['time'][k - 1]) == bits(hist[k])
    assert_bitwise(f['rho'][-1], p.q[0, [0, 50, 101], 1], 'last record against q')
    # run() continues the series of the steps before it, and a second run() of a run kept open does not start it over
    c = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, False))
    c._pre_run()
    for _ in range(3):
        c.update()
    assert c.probes.step.tolist() == [1, 2, 3] and c.probes.p is None
    quiet(c.run, keep_open=True)
    assert c.probes.step.tolist() == list(range(1, 13))
    quiet(c.run, keep_open=True)            # at max_it: no further step
    s = c.probes
    assert s.step.tolist() == list(range(1, 13))
    assert_bitwise(s.rho, f['rho'], 'update() + run() against run()')
    assert_bitwise(s.time, f['time'], 'update() + run() against run(): time')
    assert_bitwise(s.rho[-1], c.q[0, [0, 50, 101], 1], 'last record against q')
    c.set_probes([(3, 1)], pressure=False)              # a new series
    assert c.probes.step.shape == (0,) and c.probes.rho.shape == (0, 1)
    c.clear_probes()
    assert c.probes is None


def test_restored_problem_rearms_its_probes(hiplib, tmp_path):
    """Checkpoints do not carry the series: the restored problem's begins at the restart step."""
    from gapflow_amd import Problem
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, True, max_it=1000))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(4, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.probes.step.shape == (0,)
    b._advance(4, honor_stop=False)
    assert b.probes.step.tolist() == [6, 7, 8, 9]
    for name in ('time', 'rho', 'jx', 'jy', 'p'):
        assert_bitwise(getattr(b.probes, name), getattr(a.probes, name)[5:], name)


def test_refusals(hiplib):
    p = build(JOURNAL_1D)
    with pytest.raises(ValueError, match=r'\(102, 1\)'):
        p.set_probes([(1, 1), (102, 1)])
    with pytest.raises(ValueError, match=r'\(5, 3\)'):
        p.set_probes([(5, 3)])
    with pytest.raises(ValueError, match='257'):
        p.set_probes([(1 + k % 100, 1) for k in range(257)])
    with pytest.raises(ValueError):
        p.set_probes([(1.5, 1)])
    assert p.probes is None
    p.set_probes([(1 + k % 100, 1) for k in range(256)], pressure=True)       # the most a handle takes
    p._advance(3, honor_stop=False)
    assert p.probes.rho.shape == (3, 256)
    assert_bitwise(p.probes.rho[-1, :100], p.q[0, 1:101, 1], '256 probes against q')
    # the library's own checks
    import ctypes as C
    i32 = C.POINTER(C.c_int32)
    ix, iy = np.array([1, 102], dtype=np.int32), np.array([1, 1], dtype=np.int32)
    assert p._lib.gpf_probes_set(p._h, 2, ix.ctypes.data_as(i32), iy.ctypes.data_as(i32), 0) == -1
    assert b'probe 1 at cell (102, 1)' in p._lib.gpf_last_error()
    many = np.ones(257, dtype=np.int32)
    assert p._lib.gpf_probes_set(p._h, 257, many.ctypes.data_as(i32), many.ctypes.data_as(i32), 0) == -1
    assert p.probes.rho.shape == (3, 256)       # a refused call leaves the probes as they were
    p._advance(1, honor_stop=False)
    assert p.probes.step.tolist() == [1, 2, 3, 4]


SURROGATE = """
options: {silent: True, write_freq: 100}
grid: {Lx: 1470., Ly: 1., Nx: 200, Ny: 1, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P'],
       xE_D: 0.8, xW_D: 0.8}
geometry: {type: parabolic, hmin: 12., hmax: 60., U: 0.12, V: 0.}
numerics: {CFL: 0.5, adaptive: 1, tol: 1e-8, dt: 0.05, max_it: 5000}
properties: {shear: 2.15, bulk: 0., EOS: BWR, T: 1.0, rho0: 0.8}
gp:
    press: {fix_noise: True, atol: .7, rtol: 0., obs_stddev: 2.e-2, max_steps: 10, active_learning: True}
    shear: {fix_noise: True, atol: .9, rtol: 0., obs_stddev: 4.e-3, max_steps: 10, active_learning: True}
db: {init_size: 3, init_method: rand, init_width: 0.01}
"""


def test_pressure_probe_on_a_surrogate_problem_is_refused(hiplib):
    """tests/test_gpu_gp.py: test_active_learning_from_yaml's problem.  rho, jx, jy are recorded all the same."""
    import ctypes as C
    from gapflow_amd import Problem
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p = quiet(Problem.from_string, SURROGATE)
        with pytest.raises(ValueError, match='surrogate'):
            p.set_probes([(100, 1)], pressure=True)
        quiet(p._pre_run)
        ix, iy = np.array([100], dtype=np.int32), np.array([1], dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        assert p._lib.gpf_probes_set(p._h, 1, ix.ctypes.data_as(i32), iy.ctypes.data_as(i32), 1) == -1
        assert b'surrogate' in p._lib.gpf_last_error()
        cells = [(0, 1), (100, 1), (201, 1)]
        p.set_probes(cells, pressure=False)
        twin = quiet(stepped, p, cells, 2)
    assert_series_is(p.probes, twin, 'surrogate problem')


def test_slab_problems_refuse_probes_and_step_on(hiplib):
    import ctypes as C
    import torch
    from gapflow_amd.slab import SlabProblem, ThreadWorld

    def body(group):
        s = SlabProblem.from_string(SLIDER_2D, device=0, dist=group)
        with pytest.raises(NotImplementedError, match='probes: not available on a SlabProblem'):
            s.set_probes([(1, 1)])
        one = np.array([1], dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        rc = s.lib.gpf_probes_set(s._h, 1, one.ctypes.data_as(i32), one.ctypes.data_as(i32), 0)
        msg = s.lib.gpf_last_error().decode()
        s.pre_run()
        s.advance(3)
        return rc, msg, int(s.state().step)

    for rc, msg, step in quiet(ThreadWorld(2, torch).run, body):
        assert rc == -5 and 'this handle is a slab' in msg and step == 3
    with pytest.raises(NotImplementedError, match='probes: not available on a SlabProblem'):
        SlabProblem.from_string(SLIDER_2D.replace('silent: True', 'silent: True, probes: [[1, 1]]'), device=0, dist=object())
