"""Film integrals (gpf_integrals_*, Problem.set_integrals / integrals / film_integrals, options.integrals): load, its moments,
the pressure's push on the profiled wall, wall friction and flow rates through cross-sections, reduced on the device while
gpf_step advances whole batches.

The yardstick for the VALUES is a second, identical Problem advanced by update() one step at a time with q read after every
step: per step the integrands come from oracle/closures.py (eos_pressure, piezoviscosity, stress_bottom / stress_top with
slip="top") on the twin's q, topo.full, slip-length field, U and V, and are summed with math.fsum.  Tolerance per quantity:
(1e-12 + n eps) sum|term| dA -- 1e-12 is the per-cell tolerance the project holds cell_fields and the device EOS to
(test_closure_fields_match_reference_outputs, test_eos_pressure_and_sound_speed), n eps (n cells summed, eps = 2^-53) bounds
the rounding of ANY summation order; for the flow rates the integrand part is 4 eps (two products).  Everything else is held
bit for bit: a record is a pure function of the state, and recording only reads.  Reference: none (post-processing there).

The load's pressure is film_pressure (csrc/integral_kernels.hip): Dowson-Higginson with the reference's own divisions, because
eos_pressure<EOS_DH>'s rho * (1 / rho0) put the pressure sums of the stiff cases (C1 = 3.5e10, P0 = 1e5) at 40 to 160 times this
tolerance (measured).  Measured figures: the docstring of test_values_match_the_oracle_sums."""
import contextlib
import functools
import io
import math
import os
import warnings

import numpy as np
import pytest

import test_gpu_probes as tp
from test_gpu_probes import (ASPERITY_2D, JOURNAL_1D, SCALARS, SLIDER_2D, SURROGATE, THINNING, assert_bitwise, assert_same_scalars,
                             bits, quiet, scalars_of)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SUMS = ('load', 'load_x', 'load_y', 'p_hx', 'p_hy', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')

# Ny = 300: off the small-grid kernel, 150 column pairs; Roelands piezo-viscosity as tests/test_gpu_profiles.py: ASPERITY_2D has
# it.  (A thread owns column PAIRS, so 300 columns are one pair per thread for 150 threads: the case in which a thread walks on
# to a second pair is STRIDED below.)
PIEZO_WIDE = """
options: {silent: True}
grid: {Nx: 24, Ny: 300, Lx: 0.006, Ly: 0.06, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 876.,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}
numerics: {CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, max_it: 100000}
properties: {EOS: DH, shear: 0.0794, bulk: 0.02, rho0: 877.7007, P0: 1.e8, C1: 3.5e8, piezo: {name: Roelands, mu_inf: 1.e-3, p_ref: 1.96e8, z: 0.68}}
"""
# Ny = 601 > 512 and odd: a thread walks more than one column PAIR, the last pair is half a pair
STRIDED = PIEZO_WIDE.replace('Nx: 24, Ny: 300', 'Nx: 6, Ny: 601').replace('Lx: 0.006, Ly: 0.06', 'Lx: 0.0015, Ly: 0.12')
# a per-cell slip length (extra_field), as test_closure_fields_match_reference_outputs builds its problem
SLIP_FIELD = """
options: {silent: True}
grid: {Nx: 16, Ny: 40, Lx: 0.004, Ly: 0.01, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 876.,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}
numerics: {CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, max_it: 100000}
properties: {EOS: DH, shear: 0.0794, bulk: 0.02, rho0: 877.7007}
"""

# name: (input, steps, slip-length field, sections_x, sections_y); None: the default sections
CASES = {'small-1d': (JOURNAL_1D, 50, False, None, None),
         'slider-rowcoef': (SLIDER_2D, 12, False, [1, 64, 65, 128], [1, 2, 127, 128, 129, 130]),
         'asperity-planes': (ASPERITY_2D, 8, False, None, None),
         'piezo-wide': (PIEZO_WIDE, 6, False, [1, 12, 24], [1, 256, 257, 300]),
         'slip-field': (SLIP_FIELD, 5, True, [3], [1, 2, 3, 4, 37, 38, 39, 40]),
         'strided-pairs': (STRIDED, 4, False, None, [1, 512, 513, 514, 600, 601])}
NAMES = list(CASES)


def build(name):
    from gapflow_amd import Problem
    from gapflow_amd.io import read_yaml_input
    text, _, slip, _, _ = CASES[name]
    if not slip:
        return tp.build(text)
    with io.StringIO(text) as f:
        d = read_yaml_input(f)
    g = d['grid']
    x = np.linspace(0., 1., g['Nx'] + 2)[:, None]
    y = np.linspace(0., 1., g['Ny'] + 2)[None, :]
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'],
                    extra_field=1.e-6 * (1. + np.sin(3. * x) * np.cos(2. * y)))
        p._pre_run()
    return p


def armed(name, every=1):
    p = build(name)
    _, _, _, sx, sy = CASES[name]
    p.set_integrals(every, sx, sy)
    return p


def oracle_record(p):
    """name -> (value, tolerance) for the problem's current state: fsum of the oracle's integrands over the interior."""
    from gapflow_amd import _lib
    from gapflow_amd.topography import create_midpoint_grid
    from oracle import closures as ocl
    q, topo, Ls = np.array(p.q), np.array(p.topo.full[:3]), np.array(p._extra[0])
    prop = dict(_lib.EOS_DEFAULTS[p.prop['EOS']], **p.prop)
    U, V, zeta = p.geo['U'], p.geo['V'], p.prop['bulk']
    dx, dy = p.grid['dx'], p.grid['dy']
    pr = ocl.eos_pressure(q[0], prop)
    eta = ocl.piezoviscosity(pr, p.prop['shear'], p.prop['piezo']) if 'piezo' in p.prop else p.prop['shear']
    bot = ocl.stress_bottom(q, topo, U, V, eta, zeta, Ls, slip="top")
    top = ocl.stress_top(q, topo, U, V, eta, zeta, Ls, slip="top")
    xx, yy = create_midpoint_grid(p.grid)
    terms = dict(load=pr, load_x=pr * xx, load_y=pr * yy, p_hx=pr * topo[1], p_hy=pr * topo[2], tau_xz_bot=bot[4], tau_yz_bot=bot[3],
                 tau_xz_top=top[4], tau_yz_top=top[3])
    inner = (slice(1, -1), slice(1, -1))
    out = {}
    for name, t in terms.items():
        t = np.broadcast_to(t, q[0].shape)[inner].ravel()
        out[name] = (math.fsum(t) * dx * dy, (1e-12 + t.size * EPS) * math.fsum(np.abs(t)) * dx * dy)
    sx, sy = p._integral_layout()
    for k, ix in enumerate(sx):
        t = q[1][ix, 1:-1] * topo[0][ix, 1:-1]
        out[f'flow_x[{k}]'] = (math.fsum(t) * dy, (4 * EPS + t.size * EPS) * math.fsum(np.abs(t)) * dy)
    for k, iy in enumerate(sy):
        t = q[2][1:-1, iy] * topo[0][1:-1, iy]
        out[f'flow_y[{k}]'] = (math.fsum(t) * dx, (4 * EPS + t.size * EPS) * math.fsum(np.abs(t)) * dx)
    return out


def flat(rec, k=None):
    """name -> value of record k of a series (or of a film_integrals() dict), flow sections spelled out."""
    get = (lambda n: rec[n]) if isinstance(rec, dict) else (lambda n: getattr(rec, n)[k])
    out = {n: float(get(n)) for n in SUMS}
    for n in ('flow_x', 'flow_y'):
        for j, v in enumerate(np.atleast_1d(get(n))):
            out[f'{n}[{j}]'] = float(v)
    return out


def series_arrays(s):
    return [(n, getattr(s, n)) for n in ('time',) + SUMS + ('flow_x', 'flow_y')]


def assert_same_series(a, b, what, pick=None):
    """Bitwise; `pick`: indices of a's records to hold against all of b's."""
    sel = (lambda v: v[pick]) if pick is not None else (lambda v: v)
    assert sel(a.step).tolist() == b.step.tolist(), what
    assert a.sections_x.tolist() == b.sections_x.tolist() and a.sections_y.tolist() == b.sections_y.tolist()
    for (n, x), (_, y) in zip(series_arrays(a), series_arrays(b)):
        assert_bitwise(sel(x), y, f"{what}: {n}")


@functools.lru_cache(maxsize=None)
def case_runs(name):
    """One recorded batch (every = 1), the stepped twin with its oracle sums and its film_integrals() after every step, and the
    same batch without integrals; computed once per case and only read by the tests."""
    _, n, _, _, _ = CASES[name]
    rec, twin, plain = armed(name), build(name), build(name)
    log = rec._advance(n, honor_stop=False)
    plain_log = plain._advance(n, honor_stop=False)
    twin_sections = CASES[name][3:]
    twin.set_integrals(10 ** 6, *twin_sections)         # sections only: no step of this test reaches the stride
    steps, times, oracle, now = [], [], [], []
    for _ in range(n):
        twin.update()
        steps.append(twin.step)
        times.append(twin.simtime)
        oracle.append(oracle_record(twin))
        now.append(flat(twin.film_integrals()))
    return dict(series=rec.integrals, q=rec.q.copy(), scalars=scalars_of(rec), log=[tuple(getattr(e, k) for k in SCALARS) for e in log],
                plain_q=plain.q.copy(), plain_scalars=scalars_of(plain), plain_log=[tuple(getattr(e, k) for k in SCALARS) for e in plain_log],
                twin_steps=steps, twin_times=times, oracle=oracle, now=now, twin_q=twin.q.copy())


@pytest.mark.parametrize('name', NAMES)
def test_values_match_the_oracle_sums(hiplib, name):
    """Every quantity of every recorded step within (1e-12 + n eps) sum|term| dA of the fsum of the oracle's integrands on the
    stepped twin's state; step and time equal the twin's in every bit.

    Largest |device - oracle| / tolerance measured on an MI355X, over all steps of a case:
        pressure sums (load, load_x, load_y, p_hx, p_hy)   <= 3.5e-4 in every case (small-1d 3.0e-4, slip-field 3.5e-4)
        wall stresses                                       <= 1.4e-3 (strided-pairs), <= 2.7e-4 without piezo-viscosity
        flow rates                                          <= 0.19 (strided-pairs flow_y), 0 on the x-only gaps
    With eos_pressure<EOS_DH> in film_pressure's place the pressure sums of small-1d, slider-rowcoef, asperity-planes and
    slip-field stood at 134 / 160, 40, 43 / 57 and 79 / 108 times the tolerance (a relative 1.2e-10)."""
    r = case_runs(name)
    s, n = r['series'], CASES[name][1]
    assert s.step.tolist() == r['twin_steps'] == list(range(1, n + 1))
    assert_bitwise(s.time, r['twin_times'], 'time')
    assert_bitwise(r['q'], r['twin_q'], 'final q against the stepped twin')
    assert np.all(np.isfinite(s.load))
    worst = {}
    for k in range(n):
        got = flat(s, k)
        assert sorted(got) == sorted(r['oracle'][k])
        for q, (ref, tol) in r['oracle'][k].items():
            err = abs(got[q] - ref)
            worst[q] = max(worst.get(q, 0.), err / tol if tol > 0 else (0. if err == 0 else np.inf))
    print(f"\n[{name}] largest |device - oracle| / tolerance over {n} steps: " + ', '.join(f"{q} {w:.2e}" for q, w in worst.items()))
    bad = {q: w for q, w in worst.items() if not w <= 1.0}
    assert not bad, f"{name}: outside the tolerance (error / tolerance): {bad}"


@pytest.mark.parametrize('name', NAMES)
def test_record_is_a_pure_function_of_the_state(hiplib, name):
    """The same bits from one batch, from three uneven calls, at another stride, and asked for after each single step."""
    r = case_runs(name)
    s, n = r['series'], CASES[name][1]
    parts = armed(name)
    a, b = max(1, n // 4), max(1, n // 2)
    for m in (a, b - a if b > a else 1, None):
        parts._advance(m if m is not None else n - parts.step, honor_stop=False)
    assert parts.step == n
    assert_same_series(parts.integrals, s, 'three uneven calls against one batch')
    for every in (7, 3):
        strided = armed(name, every)
        strided._advance(n, honor_stop=False)
        pick = [k for k in range(n) if (k + 1) % every == 0]
        assert strided.integrals.step.tolist() == [k + 1 for k in pick]
        assert_same_series(s, strided.integrals, f'every = 1 restricted to the multiples of {every} against every = {every}', pick=pick)
    for k in range(n):
        got, now = flat(s, k), r['now'][k]
        for q in got:
            assert bits(got[q]) == bits(now[q]), f"step {k + 1}: {q} recorded {got[q]!r}, film_integrals() on the twin {now[q]!r}"


@pytest.mark.parametrize('name', ['strided-pairs', 'slip-field', 'small-1d'])
def test_narrow_loads_give_the_same_bits(hiplib, name, monkeypatch):
    """GPF_FILM_NARROW (read when the integrals' buffers are allocated) makes k_film_partial take its 8-byte loads, which
    alignment never asks for today: the same series and the same film_integrals() in every bit as with 16-byte loads -- an odd
    Ny walked in strides (the half pair at the end), a slip-length field (the seventh plane), Ny = 1 (nothing but a half pair)."""
    r = case_runs(name)                             # wide loads: computed before the variable is set, or by an earlier test
    n = CASES[name][1]
    monkeypatch.setenv('GPF_FILM_NARROW', '1')
    p = armed(name)
    p._advance(n, honor_stop=False)
    assert_same_series(p.integrals, r['series'], '8-byte loads against 16-byte loads')
    now = flat(p.film_integrals())
    for q, v in flat(r['series'], n - 1).items():
        assert bits(v) == bits(now[q]), f"film_integrals() with 8-byte loads: {q}"
    monkeypatch.delenv('GPF_FILM_NARROW')
    p.clear_integrals()                             # the next buffers are allocated without the variable: wide again
    for q, v in flat(p.film_integrals()).items():
        if not q.startswith('flow'):                # (cleared: the default sections)
            assert bits(v) == bits(now[q]), f"film_integrals() after the variable is gone: {q}"


@pytest.mark.parametrize('name', NAMES)
def test_recording_leaves_the_run_unchanged(hiplib, name):
    """Final q, every scalar and the whole scalar log against the same batch without integrals -- on the small-grid case this
    is the cut batch against the uncut one."""
    r = case_runs(name)
    assert_bitwise(r['q'], r['plain_q'], 'final q with and without integrals')
    assert_same_scalars(r['scalars'], r['plain_scalars'], 'final scalars')
    assert len(r['log']) == len(r['plain_log']) == CASES[name][1]
    for i, (a, b) in enumerate(zip(r['log'], r['plain_log'])):
        assert_same_scalars(a, b, f"scalar record of step {i + 1}")


def test_cut_small_batches_at_a_stride_match_the_uncut_run(hiplib):
    """every = 7 on the small-grid kernel: pieces of 7, 7, ... and a remainder against one launch."""
    r = case_runs('small-1d')
    p = armed('small-1d', 7)
    log = p._advance(50, honor_stop=False)
    assert_bitwise(p.q, r['plain_q'], 'final q')
    assert_same_scalars(scalars_of(p), r['plain_scalars'], 'final scalars')
    for i, (e, b) in enumerate(zip(log, r['plain_log'])):
        assert_same_scalars(tuple(getattr(e, k) for k in SCALARS), b, f"scalar record of step {i + 1}")


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_max_it_under_honor_stop_ends_the_series(hiplib, name):
    text = CASES[name][0]
    for every, want in ((1, list(range(1, 8))), (2, [2, 4, 6]), (7, [7]), (8, [])):
        p = tp.build(text.replace('max_it: 100000', 'max_it: 7'))
        p.set_integrals(every)
        p._advance(20, honor_stop=True)
        s = p.integrals
        assert p.step == 7 and s.step.tolist() == want and s.flow_x.shape == (len(want), len(s.sections_x))
        if every == 7:
            now = flat(p.film_integrals())
            for q, v in flat(s, 0).items():
                assert bits(v) == bits(now[q]), f"last record against the state the run ended on: {q}"


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_rolled_back_step_leaves_no_record(hiplib, name):
    """tests/test_gpu_parity.py: test_invalid_state_rolls_back's way to an invalid state (an absurd time step): the scalar log
    keeps its entry for the invalid step, the series ends one entry before it."""
    from gapflow_amd import _lib
    import ctypes as C
    p = armed(name)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)          # its scalar log: one entry, flagged invalid (Problem._advance reads it)
    assert p._stop and p.step == 3
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_integrals_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 0                          # ... and no record: the series ends one entry before the log
    np.testing.assert_array_equal(p.q, good)
    assert p.integrals.step.tolist() == [1, 2, 3]
    ref = case_runs(name)['series']
    for n, x in series_arrays(p.integrals):
        assert_bitwise(x, getattr(ref, n)[:3], f"records before the rollback: {n}")


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_together_with_probes(hiplib, name):
    """Both armed: both series equal their values when armed alone, bit for bit."""
    text, n = CASES[name][0], CASES[name][1]
    cells = tp.CELLS_1D if name == 'small-1d' else tp.CELLS_2D
    both = armed(name)
    both.set_probes(cells, pressure=True)
    both._advance(n, honor_stop=False)
    assert_same_series(both.integrals, case_runs(name)['series'], 'integrals with probes armed')
    alone = tp.case_runs(name)['series']
    assert both.probes.step.tolist() == alone.step.tolist()
    for q in ('time', 'rho', 'jx', 'jy', 'p'):
        assert_bitwise(getattr(both.probes, q), getattr(alone, q), f"probes with integrals armed: {q}")


def test_refusals(hiplib):
    import ctypes as C
    from gapflow_amd import Problem, _lib
    i32 = C.POINTER(C.c_int32)
    p = tp.build(SLIDER_2D)
    with pytest.raises(ValueError, match=r'sections_x\[1\] = 129'):
        p.set_integrals(1, [1, 129])
    with pytest.raises(ValueError, match=r'sections_y\[0\] = 0'):
        p.set_integrals(1, None, [0])
    with pytest.raises(ValueError, match='stride'):
        p.set_integrals(0)
    assert p.integrals is None
    # the library's own checks name the offending section
    bad = np.array([1, 129], dtype=np.int32)
    assert p._lib.gpf_integrals_set(p._h, 1, 2, bad.ctypes.data_as(i32), 0, None) == -1
    assert b'x-section 1 at row 129' in p._lib.gpf_last_error()
    bad = np.array([131], dtype=np.int32)
    assert p._lib.gpf_integrals_set(p._h, 1, 0, None, 1, bad.ctypes.data_as(i32)) == -1
    assert b'y-section 0 at column 131' in p._lib.gpf_last_error()
    assert p._lib.gpf_integrals_set(p._h, 0, 0, None, 0, None) == -1 and b'every >= 1' in p._lib.gpf_last_error()
    assert p._lib.gpf_integrals_read(p._h, None, 0, None, None) == -5
    # an open stage-wise step
    _lib.check(p._lib.gpf_open_step(p._h))
    assert p._lib.gpf_integrals_set(p._h, 1, 0, None, 0, None) == -5 and b'stage-wise step is open' in p._lib.gpf_last_error()
    out = np.empty(32)
    assert p._lib.gpf_integrals_now(p._h, _lib.as_dp(out), 32) == -5 and b'stage-wise step is open' in p._lib.gpf_last_error()
    for i in range(2):
        _lib.check(p._lib.gpf_stage_closures(p._h))
        _lib.check(p._lib.gpf_stage_advance(p._h, i))
    sc = _lib.GpfScalars()
    _lib.check(p._lib.gpf_close_step(p._h, C.byref(sc)))
    p.set_integrals(2)                          # closed: armed; gpf_close_step itself records nothing
    assert p.integrals.step.shape == (0,)
    # shear thinning
    t = tp.build(THINNING)
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.set_integrals()
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.film_integrals()
    assert t._lib.gpf_integrals_set(t._h, 1, 0, None, 0, None) == -1 and b'shear thinning' in t._lib.gpf_last_error()
    # surrogate closures
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = quiet(Problem.from_string, SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            g.set_integrals()
        quiet(g._pre_run)
        assert g._lib.gpf_integrals_set(g._h, 1, 0, None, 0, None) == -1 and b'surrogate' in g._lib.gpf_last_error()
        assert g._lib.gpf_integrals_now(g._h, _lib.as_dp(out), 32) == -1 and b'surrogate' in g._lib.gpf_last_error()


def run_yaml(out, silent, max_it=12):
    options = (f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, integrals: 3, "
               f"integrals_sections_x: [1, 50, 100]}}")
    return JOURNAL_1D.replace("options: {silent: True}", options).replace('max_it: 100000', f'max_it: {max_it}')


def test_run_writes_integrals_npz_and_a_restored_problem_rearms(hiplib, tmp_path):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'integrals.npz'))
    assert sorted(f.files) == sorted(('step', 'time') + SUMS + ('flow_x', 'flow_y', 'sections_x', 'sections_y'))
    assert f['step'].tolist() == [3, 6, 9, 12] and f['flow_x'].shape == (4, 3) and f['flow_y'].shape == (4, 1)
    assert f['sections_x'].tolist() == [1, 50, 100] and f['sections_y'].tolist() == [1]
    ref = case_runs('small-1d')['series']                  # the same problem, every = 1, default sections (rows 1 and 100)
    assert_bitwise(f['load'], ref.load[[2, 5, 8, 11]], 'run() at stride 3 against the batch at stride 1: load')
    assert_bitwise(f['flow_x'][:, [0, 2]], ref.flow_x[[2, 5, 8, 11]], 'flow_x on rows 1 and 100')
    assert_bitwise(f['time'], ref.time[[2, 5, 8, 11]], 'time')
    # checkpoints do not carry the series: the restored problem's begins at the restart step
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(7, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.integrals.step.shape == (0,) and b.integrals.sections_x.tolist() == [1, 50, 100]
    b._advance(7, honor_stop=False)
    assert a.integrals.step.tolist() == [3, 6, 9, 12] and b.integrals.step.tolist() == [6, 9, 12]
    for n, x in series_arrays(b.integrals):
        assert_bitwise(x, dict(series_arrays(a.integrals))[n][1:], f"restored against continued: {n}")
    b.clear_integrals()
    assert b.integrals is None
