"""Running field statistics (gpf_stats_*, Problem.set_statistics / statistics) on the device, against the states themselves.

The reference of every plane is tests/statistics_cases.py: welford -- the kernel's recurrences restated in NumPy -- applied to the
states downloaded after single update() calls.  rho, jx, jy are the operands themselves, so their planes are compared BITWISE
over the whole ghosted field; p is compared bitwise with the restatement applied to the probes' p at 256 cells (the probes call
the same device function), and over the whole field with the restatement applied to the oracle's EOS pressure at 1e-9 of the
field scale, the project's device-parity bound (Dowson-Higginson amplifies the last bit of the reciprocal, 3.3f)."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest

import statistics_cases as sc
import test_gpu_probes as tp

pytestmark = pytest.mark.gpu

SCALARS = tp.SCALARS
FIELDS = ('p', 'rho', 'jx', 'jy')
STATE = {'rho': 0, 'jx': 1, 'jy': 2}
P_PARITY = 1e-9

# Dirichlet / Neumann edges in x, periodic in y, one asperity (gap planes), V != 0: nothing is uniform along either axis
TWO_D = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: 0.02, Ly: 0.03, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P'], xE_D: 877.7007, xW_D: 877.7007}}
geometry: {{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.05}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1e-14, dt: 2.e-9, max_it: {max_it}}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}}
"""
ONE_D = tp.JOURNAL_1D                   # Nx = 100, Ny = 1: the one-workgroup kernel
ONE_D_LONG = tp.JOURNAL_1D.replace('Nx: 100', 'Nx: 500').replace('dx: 1.e-5', 'dx: 2.e-6')      # 502 x 3 cells: launch per step
NSTEPS = 12


def text_2d(ny=45, max_it=100000):
    return TWO_D.format(nx=37, ny=ny, max_it=max_it)       # 39 x 47 ghosted cells: above the one-workgroup limit of 1200


quiet, build, bits, assert_bitwise, scalars_of = tp.quiet, tp.build, tp.bits, tp.assert_bitwise, tp.scalars_of


def probe_cells(nx, ny):
    """256 cells: the four corners, both ghost rows and columns, the last pair of every tenth row, a spread of interior cells."""
    cells = [(0, 0), (0, ny + 1), (nx + 1, 0), (nx + 1, ny + 1)]
    cells += [(ix, iy) for ix in (0, nx + 1) for iy in range(1, ny + 1, 3)]
    cells += [(ix, iy) for iy in (0, ny + 1) for ix in range(1, nx + 1, 2)]
    cells += [(ix, iy) for ix in range(1, nx + 1, 10) for iy in (ny - 1, ny)]
    k = 0
    while len(cells) < 256:
        c = (1 + (7 * k) % nx, 1 + (11 * k + k // nx) % ny)
        if c not in cells:
            cells.append(c)
        k += 1
    assert len(set(cells)) == 256
    return cells


def planes_of(stats, field):
    return {k: stats[f'{field}_{k}'] for k in sc.QUANTITIES}


def assert_planes(stats, field, want, what):
    for k in sc.QUANTITIES:
        assert_bitwise(stats[f'{field}_{k}'], want[k], f"{what}: {field}_{k}")
    assert_bitwise(stats[f'{field}_var'], want['m2'] / want['count'], f"{what}: {field}_var")


def assert_state_planes(stats, states, what, fields=('rho', 'jx', 'jy')):
    assert stats['count'] == len(states), what
    for f in fields:
        assert_planes(stats, f, sc.welford([q[STATE[f]] for q in states]), what)


def stepped_run(text, fields=FIELDS, cells=None, every=1, after=0, n=NSTEPS, arm=True):
    """n single update() calls, q downloaded after each: the states, the times, the statistics, the probes, the end of the run."""
    p = build(text)
    if cells is not None:
        p.set_probes(cells, pressure=True)
    if arm:
        p.set_statistics(every, fields, after)
    states, times = [], []
    for _ in range(n):
        p.update()
        states.append(p.q.copy())
        times.append(p.simtime)
    return dict(states=states, times=times, stats=p.statistics, probes=p.probes, q=p.q.copy(), scalars=scalars_of(p), prop=p.prop, cells=cells)


@functools.lru_cache(maxsize=None)
def case_one():
    """Case 1's run, computed once and only read: every = 1, all four fields, 256 probes, 12 single updates on 37 x 45."""
    return stepped_run(text_2d(45), cells=probe_cells(37, 45))


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2. the launch-per-step path
# ---------------------------------------------------------------------------------------------------------------------------
def test_planes_are_the_restatement_on_the_stepped_states(hiplib):
    r = case_one()
    s = r['stats']
    assert s['count'] == NSTEPS and s['first_step'] == 1 and s['last_step'] == NSTEPS
    assert bits(s['t_first']) == bits(r['times'][0]) and bits(s['t_last']) == bits(r['times'][-1])
    assert s['rho_mean'].shape == (39, 47)
    assert_state_planes(s, r['states'], '37 x 45, every = 1')
    # p at the probes' cells: the same device function, the same bits
    ix, iy = np.array(r['cells']).T
    want = sc.welford(list(r['probes'].p))
    for k in sc.QUANTITIES:
        assert_bitwise(s[f'p_{k}'][ix, iy], want[k], f"p_{k} at the 256 probe cells")
    # p over the whole field: the oracle's EOS pressure, at the device-parity bound
    from oracle.closures import eos_pressure
    ref = sc.welford([eos_pressure(q[0], r['prop']) for q in r['states']])
    scale = np.abs(ref['mean']).max()
    err = np.abs(s['p_mean'] - ref['mean']).max() / scale
    print(f"\n[p_mean against the oracle's EOS pressure] max |difference| / scale = {err:.3e} (bound {P_PARITY:.0e})")
    assert err <= P_PARITY
    assert np.all(s['p_min'] <= s['p_mean']) and np.all(s['p_mean'] <= s['p_max']) and np.all(s['p_m2'] >= 0)
    assert np.any(s['rho_m2'] > 0), 'the run does move'


@pytest.mark.parametrize('text,shape', [(text_2d(44), (39, 46)), (ONE_D_LONG, (502, 3))], ids=['even-ny', '1d-500'])
def test_even_ny_and_one_dimension(hiplib, text, shape):
    r = stepped_run(text, fields=('rho', 'jx', 'jy'))
    assert r['stats']['rho_max'].shape == shape and 'p_mean' not in r['stats']
    assert_state_planes(r['stats'], r['states'], str(shape))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. batches, stride, after
# ---------------------------------------------------------------------------------------------------------------------------
def test_batch_stride_and_after(hiplib):
    r = case_one()
    p = build(text_2d(45))
    p.set_statistics(every=3, after=2)
    p._advance(NSTEPS, honor_stop=False)
    s = p.statistics
    assert (s['count'], s['first_step'], s['last_step']) == (4, 3, 12)
    assert bits(s['t_first']) == bits(r['times'][2]) and bits(s['t_last']) == bits(r['times'][11])
    picked = [r['states'][k - 1] for k in (3, 6, 9, 12)]
    assert_state_planes(s, picked, 'one batch of 12, every = 3, after = 2')
    ix, iy = np.array(r['cells']).T
    want = sc.welford([r['probes'].p[k - 1] for k in (3, 6, 9, 12)])
    for k in sc.QUANTITIES:
        assert_bitwise(s[f'p_{k}'][ix, iy], want[k], f"p_{k} at the probe cells")
    single = stepped_run(text_2d(45), every=3, after=2)['stats']
    assert single['count'] == 4
    for f in FIELDS:
        assert_planes(single, f, dict(planes_of(s, f), count=4), 'twelve single updates against one batch')
    # after beyond a multiple: steps 6, 9, 12 (not 3; 4 is no multiple)
    p.set_statistics(every=3, after=4)
    assert p.statistics is None
    p._advance(NSTEPS, honor_stop=False)        # steps 13 .. 24, armed at 12: 15, 18, 21, 24
    assert (p.statistics['count'], p.statistics['first_step'], p.statistics['last_step']) == (4, 15, 24)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. recording only reads
# ---------------------------------------------------------------------------------------------------------------------------
def test_recording_leaves_the_run_unchanged(hiplib):
    r = case_one()
    plain = stepped_run(text_2d(45), arm=False)
    assert_bitwise(r['q'], plain['q'], 'q after 12 steps, with and without statistics')
    tp.assert_same_scalars(r['scalars'], plain['scalars'], 'scalars')
    for a, b in zip(r['states'], plain['states']):
        assert_bitwise(a, b, 'every state on the way')


# ---------------------------------------------------------------------------------------------------------------------------
# 5, 6. the small grid: the cut batch, the union of the cuts
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_states(n):
    """n single updates of the 1-D problem: the states, the final q and scalars; SMALL_P[k]: the probes' p of step k + 1 along iy = 1."""
    p = build(ONE_D)
    p.set_probes([(ix, 1) for ix in range(102)], pressure=True)
    states = []
    for _ in range(n):
        p.update()
        states.append(p.q.copy())
    SMALL_P[:] = list(p.probes.p)
    return states, p.q.copy(), scalars_of(p)


SMALL_P = []


def test_small_grid_batch_is_cut_at_the_recorded_steps(hiplib):
    states, q, scalars = small_states(30)
    p = build(ONE_D)
    p.set_statistics(every=4)
    p._advance(20, honor_stop=False)
    s = p.statistics
    assert (s['count'], s['first_step'], s['last_step']) == (5, 4, 20)
    assert_state_planes(s, [states[k - 1] for k in (4, 8, 12, 16, 20)], 'small grid, every = 4, one call of 20')
    assert_bitwise(p.q, states[19], 'q against the unarmed run')
    want = sc.welford([SMALL_P[k - 1] for k in (4, 8, 12, 16, 20)])
    for k in sc.QUANTITIES:
        assert_bitwise(s[f'p_{k}'][:, 1], want[k], f"p_{k} along iy = 1 against the probes' p")


def test_union_cut_keeps_each_series_as_it_is_alone(hiplib):
    states, q, scalars = small_states(30)
    ones = np.ones((100, 1))

    def run(integrals=False, weighted=False, stats=False):
        p = build(ONE_D)
        if integrals:
            p.set_integrals(2)
        if weighted:
            p.set_weighted_integrals(ones, every=3)
        if stats:
            p.set_statistics(every=5)
        p._advance(30, honor_stop=False)
        return p

    both, a, b, c = run(True, True, True), run(integrals=True), run(weighted=True), run(stats=True)
    assert_bitwise(both.q, q, 'q against the unarmed run')
    tp.assert_same_scalars(scalars_of(both), scalars, 'scalars against the unarmed run')
    assert both.integrals.step.tolist() == a.integrals.step.tolist() == list(range(2, 31, 2))
    for k in ('time', 'load', 'load_x', 'p_hx', 'tau_xz_bot', 'tau_xz_top', 'flow_x', 'flow_y'):
        assert_bitwise(getattr(both.integrals, k), getattr(a.integrals, k), f"film integrals at 2: {k}")
    assert both.weighted_integrals.step.tolist() == b.weighted_integrals.step.tolist() == list(range(3, 31, 3))
    for k in ('time', 'p', 'h', 'rho_h', 'jx_h', 'tau_xz_bot', 'tau_xz_top'):
        assert_bitwise(getattr(both.weighted_integrals, k), getattr(b.weighted_integrals, k), f"weighted integrals at 3: {k}")
    sb, sc_ = both.statistics, c.statistics
    assert sb['count'] == sc_['count'] == 6 and sb['last_step'] == 30
    for f in FIELDS:
        assert_planes(sb, f, dict(planes_of(sc_, f), count=6), 'statistics at 5, together against alone')
    assert_state_planes(sb, [states[k - 1] for k in range(5, 31, 5)], 'statistics at 5 against the restatement')


# ---------------------------------------------------------------------------------------------------------------------------
# 7, 8. a batch that stops on the device; rollback
# ---------------------------------------------------------------------------------------------------------------------------
def test_batch_that_stops_at_max_it(hiplib):
    r = case_one()
    p = build(text_2d(45, max_it=7))
    p.set_statistics(every=2)
    p._advance(NSTEPS, honor_stop=True)
    assert p.step == 7
    s = p.statistics
    assert (s['count'], s['first_step'], s['last_step']) == (3, 2, 6)
    assert bits(s['t_last']) == bits(r['times'][5])
    assert_state_planes(s, [r['states'][k - 1] for k in (2, 4, 6)], 'stopped at max_it = 7, every = 2')


@pytest.mark.parametrize('text', [ONE_D, text_2d(45)], ids=['small-1d', '37x45'])
def test_rolled_back_step_touches_nothing(hiplib, text):
    p = build(text)
    p.set_statistics(every=1)
    p._advance(3, honor_stop=False)
    before = p.statistics
    p.q[0, 5, 1] = -p.q[0, 5, 1]                # a negative density: the next step is flagged invalid and rolled back
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    after = p.statistics
    assert after['count'] == before['count'] == 3 and after['last_step'] == 3
    assert bits(after['t_last']) == bits(before['t_last'])
    for f in FIELDS:
        assert_planes(after, f, dict(planes_of(before, f), count=3), 'planes after the rollback')


# ---------------------------------------------------------------------------------------------------------------------------
# 9. wide against narrow accesses
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ny', [45, 44])
def test_narrow_accesses_give_the_same_bits(hiplib, monkeypatch, ny):
    wide = build(text_2d(ny))
    wide.set_statistics(every=1)
    monkeypatch.setenv('GPF_FILM_NARROW', '1')
    narrow = build(text_2d(ny))
    narrow.set_statistics(every=1)              # the switch is read here
    monkeypatch.delenv('GPF_FILM_NARROW')
    for p in (wide, narrow):
        p._advance(NSTEPS, honor_stop=False)
    sw, sn = wide.statistics, narrow.statistics
    assert sw['count'] == sn['count'] == NSTEPS
    for f in FIELDS:
        assert_planes(sn, f, dict(planes_of(sw, f), count=NSTEPS), f"Ny = {ny}: 8-byte against 16-byte accesses")
    if ny == 45:
        assert_state_planes(sn, case_one()['states'], 'narrow accesses against the restatement')


# ---------------------------------------------------------------------------------------------------------------------------
# 10. the stage-wise pipeline
# ---------------------------------------------------------------------------------------------------------------------------
def test_stage_wise_steps(hiplib):
    r = stepped_run(tp.THINNING, n=5)
    assert r['stats']['count'] == 5 and r['stats']['rho_mean'].shape == (50, 12)
    assert_state_planes(r['stats'], r['states'], 'Eyring thinning, 48 x 10, 5 closed steps')


# ---------------------------------------------------------------------------------------------------------------------------
# 11. arming again, starting over
# ---------------------------------------------------------------------------------------------------------------------------
def info(p):
    cnt, first, last = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert p._lib.gpf_stats_info(p._h, C.byref(cnt), C.byref(first), C.byref(last), None, None) == 0
    return cnt.value, first.value, last.value


def test_arming_again_and_restarts_begin_a_new_window(hiplib):
    states, _, _ = small_states(30)
    p = build(ONE_D)
    p.set_statistics(every=1, fields=('rho',))
    assert p.statistics is None
    p._advance(4, honor_stop=False)
    assert p.statistics['count'] == 4
    p.set_statistics(every=1, fields=('rho', 'jx'))         # again: from scratch
    assert info(p)[0] == 0 and p.statistics is None
    p._advance(2, honor_stop=False)
    s = p.statistics
    assert (s['count'], s['first_step'], s['last_step']) == (2, 5, 6) and 'jx_mean' in s and 'p_mean' not in s
    assert_state_planes(s, states[4:6], 'window armed at step 4', fields=('rho', 'jx'))
    # another state from another handle (gpf_resample): the window restarts where the step count stands
    src = build(ONE_D)
    assert p._lib.gpf_resample(p._h, src._h) == 0
    assert info(p)[0] == 0 and p.statistics is None
    p._mark_device_advanced()
    p._advance(2, honor_stop=False)
    assert info(p) == (2, 7, 8)
    # init_from after steps starts the run over, and the window with it
    p.init_from(src)
    assert p.step == 0 and info(p)[0] == 0 and p.statistics is None
    got = []
    for _ in range(3):
        p.update()
        got.append(p.q.copy())
    assert_state_planes(p.statistics, got, 'after init_from', fields=('rho', 'jx'))
    p._pre_run()
    assert info(p)[0] == 0 and p.statistics is None
    p.clear_statistics()
    assert p.statistics is None and p._lib.gpf_stats_info(p._h, None, None, None, None, None) == -5


# ---------------------------------------------------------------------------------------------------------------------------
# 12. refusals through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_library_refusals(hiplib):
    from gapflow_amd import _lib
    p = build(ONE_D)
    lib = p._lib
    assert lib.gpf_stats_set(None, 1, 0, 15) == -1
    assert lib.gpf_stats_set(p._h, 0, 0, 15) == -1 and b'every >= 1' in lib.gpf_last_error()
    assert lib.gpf_stats_set(p._h, 1, -1, 15) == -1 and b'after >= 0' in lib.gpf_last_error()
    for mask in (0, 16, -1):
        assert lib.gpf_stats_set(p._h, 1, 0, mask) == -1 and b'field mask' in lib.gpf_last_error()
    out = np.zeros(p._shape)
    assert lib.gpf_stats_read(p._h, 1, 0, _lib.as_dp(out), out.size) == -5 and b'armed' in lib.gpf_last_error()
    p.set_statistics(every=2, fields=('rho',))
    assert lib.gpf_stats_read(p._h, 1, 0, _lib.as_dp(out), out.size) == -5 and b'nothing has been recorded' in lib.gpf_last_error()
    p._advance(2, honor_stop=False)
    assert lib.gpf_stats_read(p._h, 1, 0, _lib.as_dp(out), out.size) == 0 and np.array_equal(out, p.q[0])
    assert lib.gpf_stats_read(p._h, 0, 0, _lib.as_dp(out), out.size) == -1 and b'not among the armed' in lib.gpf_last_error()
    assert lib.gpf_stats_read(p._h, 1, 4, _lib.as_dp(out), out.size) == -1
    assert lib.gpf_stats_read(p._h, 1, 0, _lib.as_dp(out), out.size - 1) == -1
    # a slab handle: this problem's configuration with a halo row
    cfg = _lib.GpfConfig.from_buffer_copy(p._cfg)
    cfg.halo_lo = 1
    slab = C.c_void_p()
    assert lib.gpf_create(C.byref(cfg), C.byref(slab)) == 0
    try:
        assert lib.gpf_stats_set(slab, 1, 0, 2) == -5 and b'this handle is a slab' in lib.gpf_last_error()
    finally:
        lib.gpf_destroy(slab)
    # an armed member
    other = build(ONE_D)
    handles = (C.c_void_p * 2)(other._h.value, p._h.value)
    e = C.c_void_p()
    assert lib.gpf_ensemble_create(handles, 2, C.byref(e)) == -1
    assert b'member 1: statistics are armed on it' in lib.gpf_last_error()
    from gapflow_amd import Ensemble
    with pytest.raises(NotImplementedError, match='member 1: statistics are armed'):
        Ensemble([other, p])


def test_pressure_statistics_need_the_equation_of_state(hiplib):
    """tests/test_gpu_probes.py: SURROGATE (pressure and shear from Gaussian processes): p is refused, rho, jx, jy are recorded."""
    from gapflow_amd import Problem
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p = quiet(Problem.from_string, tp.SURROGATE)
        with pytest.raises(ValueError, match='surrogate'):
            p.set_statistics(every=1)
        quiet(p._pre_run)
        assert p._lib.gpf_stats_set(p._h, 1, 0, 15) == -1 and b'surrogate' in p._lib.gpf_last_error()
        p.set_statistics(every=1, fields=('rho', 'jx', 'jy'))
        states = []
        for _ in range(2):
            quiet(p.update)
            states.append(p.q.copy())
    assert_state_planes(p.statistics, states, 'surrogate problem, without p')


# ---------------------------------------------------------------------------------------------------------------------------
# 13. output
# ---------------------------------------------------------------------------------------------------------------------------
def test_run_writes_statistics_npz(hiplib, tmp_path):
    from gapflow_amd import Problem
    options = f"options: {{output: {tmp_path / 'run'}, write_freq: 5, use_tstamp: False, silent: False, statistics: 3, statistics_fields: [p, rho], statistics_after: 3}}"
    text = ONE_D.replace("options: {silent: True}", options).replace('max_it: 100000', 'max_it: 12')
    p = quiet(Problem.from_string, text)
    quiet(p.run)
    s = p.statistics
    assert (s['count'], s['first_step'], s['last_step']) == (3, 6, 12)
    f = np.load(os.path.join(p.outdir, 'statistics.npz'))
    assert sorted(f.files) == sorted(['fields'] + list(s))
    assert f['fields'].tolist() == ['p', 'rho'] and 'jx_mean' not in f.files
    for k, v in s.items():
        if isinstance(v, np.ndarray):
            assert_bitwise(f[k], v, f"statistics.npz: {k}")
        else:
            assert f[k].shape == () and bits(float(f[k])) == bits(float(v)), k


def test_restored_problem_rearms_and_starts_a_new_window(hiplib, tmp_path):
    from gapflow_amd import Problem
    text = ONE_D.replace("options: {silent: True}", "options: {silent: True, statistics: 2, statistics_fields: [rho]}")
    a = quiet(Problem.from_string, text)
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b._stats_every == 2 and b.statistics is None
    b._advance(4, honor_stop=False)
    s = b.statistics
    assert (s['count'], s['first_step'], s['last_step']) == (2, 6, 8)
    states, _, _ = small_states(30)
    assert_state_planes(s, [states[5], states[7]], 'restored at step 5', fields=('rho',))
