"""Resampling a state onto another grid on the device (gpf_resample, Problem.init_from).

Values are held against the NumPy restatement of tests/resample_cases.py -- gapflow_amd.resample.axis_weights, the four-term blend,
the division by the destination's gap, then the destination's own edge rules for the ghost cells -- to 1e-13 of each component's
largest magnitude, ghost cells included: a blend of four like-sized terms and one division lose a few ulp, a margin of about 100.
The sources are problems advanced 20 steps from the uniform field over a gap that varies along both axes (one cosine asperity),
so that rho, jx and jy all vary along both; they are built once and only read."""
import contextlib
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import reference_suite as rs
import resample_cases as rc

pytestmark = pytest.mark.gpu

SCALARS = ('step', 'simtime', 'dt', 'ekin', 'ekin_old', 'residual', 'v_max', 'v_sound', 'mass', 'invalid', 'converged')
TOL = 1e-13

PERIODIC = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: 1.e-3, Ly: 8.e-4, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: asperity, hmin: 4.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, dt: 1.e-10, max_it: {max_it}}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007, P0: 101325., C1: 3.5e10, C2: 1.23}}
"""
# an inclined slider between Dirichlet (rho) / Neumann (jx, jy) edges in x and Neumann edges in y
SLIDER = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: 1.e-3, Ly: 8.e-4, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 876.,
       yS: ['N', 'N', 'N'], yN: ['N', 'N', 'N']}}
geometry: {{type: inclined, hmin: 5.e-6, hmax: 1.e-5, U: 0.5, V: 0.1}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, dt: 1.e-10, max_it: {max_it}}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007, P0: 101325., C1: 3.5e10, C2: 1.23}}
"""
JOURNAL_1D = rs.JOURNAL_1D
JOURNAL_1D_COARSE = JOURNAL_1D.replace('Nx: 100', 'Nx: 50').replace('dx: 1.e-5', 'dx: 2.e-5')


def text_of(template, shape, max_it=100000):
    if template in (JOURNAL_1D, JOURNAL_1D_COARSE):
        return template
    return template.format(nx=shape[0], ny=shape[1], max_it=max_it)


# name: (source input, destination input).  'strided': Ny = 601 > 512 and odd -- a thread walks on to a second column pair, and
# the last pair is half a pair
CASES = {'a': ((JOURNAL_1D_COARSE, None), (JOURNAL_1D, None)),
         'b': ((PERIODIC, (12, 10)), (PERIODIC, (30, 25))),
         'c': ((SLIDER, (16, 8)), (SLIDER, (40, 24))),
         'd': ((PERIODIC, (30, 25)), (PERIODIC, (12, 10))),
         'e': ((PERIODIC, (12, 10)), (PERIODIC, (48, 40))),
         'f': ((PERIODIC, (16, 8)), (PERIODIC, (16, 8))),
         'strided': ((PERIODIC, (4, 24)), (PERIODIC, (6, 601)))}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(text):
    from gapflow_amd import Problem
    return quiet(Problem.from_string, text)


def advance(p, n):
    if p.step is None:
        p._pre_run()
    for _ in range(n):
        p.update()
    return p


@functools.lru_cache(maxsize=None)
def source(template, shape):
    """The source of a case: 20 steps from the uniform field.  Shared, and only ever read."""
    return advance(build(text_of(template, shape)), 20)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bitwise(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    same = bits(a) == bits(b)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ, max |difference| {np.nanmax(np.abs(a - b)):.3e}"


def scalars_of(p):
    sc = p._scalars()
    return tuple(getattr(sc, k) for k in SCALARS)


def gap_of(p):
    from gapflow_amd import _lib
    return p._download(_lib.FIELD_TOPO, 3)[0]


def restatement(src, dst):
    """What dst.init_from(src) must leave in dst.q, ghost cells included."""
    interior = rc.numpy_resample(np.array(src.q), gap_of(src), gap_of(dst), (src.grid['dx'], src.grid['dy']), (dst.grid['dx'], dst.grid['dy']))
    rules, values = dst._edge_rules()
    return rc.fill_ghosts(interior, rules, values)


def resampled(case):
    (st, ss), (dt, ds) = CASES[case]
    src = source(st, ss)
    dst = build(text_of(dt, ds))
    dst.init_from(src)
    return src, dst


# ---- values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(CASES))
def test_values_match_the_numpy_restatement(hiplib, case):
    src, dst = resampled(case)
    got, want = np.array(dst.q), restatement(src, dst)
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    for c, name in enumerate(('rho', 'jx', 'jy')):
        scale = np.abs(want[c]).max()
        err = np.abs(got[c] - want[c]).max()
        print(f"\n[resample {case}] {name}: max error {err / scale if scale else err:.2e} of max|{name}| = {scale:.3e}")
        assert err <= TOL * scale, f"case {case}, {name}: {err:.3e} > {TOL} x {scale:.3e}"
    if CASES[case][0][0] is PERIODIC:       # these sources do vary along both axes
        s = np.array(src.q)[:, 1:-1, 1:-1]
        for c in range(3):
            assert np.ptp(s[c], axis=0).max() > 0 and np.ptp(s[c], axis=1).max() > 0


def test_identity_keeps_rho_bitwise_and_momenta_within_4_ulp(hiplib):
    src, dst = resampled('f')
    got, q = np.array(dst.q), np.array(src.q)
    assert_bitwise(got[0, 1:-1, 1:-1], q[0, 1:-1, 1:-1], 'rho, interior')
    rules, values = dst._edge_rules()
    assert_bitwise(got[0], rc.fill_ghosts(q[:, 1:-1, 1:-1], rules, values)[0], 'rho, ghost cells by the edge rules')
    for c, name in ((1, 'jx'), (2, 'jy')):
        ulps = np.abs(got[c, 1:-1, 1:-1] - q[c, 1:-1, 1:-1]) / np.spacing(np.abs(q[c, 1:-1, 1:-1]))
        assert ulps.max() <= 4, f"{name}: {ulps.max()} ulp"


def test_narrow_stores_equal_wide_stores_bitwise(hiplib, monkeypatch):
    src, wide = resampled('b')
    monkeypatch.setenv('GPF_FILM_NARROW', '1')
    _, narrow = resampled('b')
    monkeypatch.delenv('GPF_FILM_NARROW')
    assert_bitwise(narrow.q, wide.q, '8-byte against 16-byte stores')


# ---- the destination afterwards, the source afterwards ------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(30, 25), (48, 40)], ids=['one-workgroup', 'k_step2'])
def test_destination_continues_like_a_twin_given_the_same_field(hiplib, shape, tmp_path):
    """dst after init_from against a twin that had the downloaded field assigned to q: 8 steps of run(), then q, dt, the scalars
    and the history (rows at steps 0, 4, 8) are the same bits.  A third problem that had already taken steps starts over at
    step 0 and joins them."""
    src = source(PERIODIC, (12, 10))
    text = text_of(PERIODIC, shape, max_it=8)
    dst, twin, late = (build(text.replace('silent: True', f'silent: False, output: {tmp_path / name}, use_tstamp: False, write_freq: 4'))
                       for name in ('dst', 'twin', 'late'))
    dst.init_from(src)
    field = np.array(dst.q)
    twin.q[...] = field
    advance(late, 3)
    late.init_from(src)
    assert late.step == 0 and late.simtime == 0.
    assert_bitwise(late.q, field, 'q of a problem that had taken steps before')
    for p in (dst, twin, late):
        quiet(p.run)
        assert p.step == 8
    for other, what in ((twin, 'twin'), (late, 'late')):
        assert_bitwise(dst.q, other.q, f'q after 8 steps ({what})')
        assert_bitwise(dst.dt, other.dt, f'dt ({what})')
        assert scalars_of(dst) == scalars_of(other), what
        assert dst.history == other.history, what
    assert dst.history['step'] == [0, 4, 8]


def test_the_source_is_only_read(hiplib):
    a, b = (advance(build(text_of(PERIODIC, (12, 10))), 20) for _ in range(2))
    dst = build(text_of(PERIODIC, (30, 25)))
    dst.init_from(a)
    assert_bitwise(a.q, b.q, 'q of the source')
    assert scalars_of(a) == scalars_of(b)
    assert (a.step, a.simtime, a.dt, a.residual) == (b.step, b.simtime, b.dt, b.residual)
    advance(a, 4)
    advance(b, 4)
    assert_bitwise(a.q, b.q, 'q of the source, 4 steps on')
    assert scalars_of(a) == scalars_of(b)


def test_series_start_afresh(hiplib):
    src = source(PERIODIC, (12, 10))
    dst = build(text_of(PERIODIC, (30, 25)))
    dst.set_extrema(1)
    dst.set_probes([[3, 4]])
    dst.set_integrals(2)
    advance(dst, 5)
    assert len(dst.extrema.step) == 5 and len(dst.probes.step) == 5 and len(dst.integrals.step) == 2
    dst.init_from(src)
    assert len(dst.extrema.step) == 0 and len(dst.probes.step) == 0 and len(dst.integrals.step) == 0
    advance(dst, 2)
    assert dst.extrema.step.tolist() == [1, 2] and dst.probes.step.tolist() == [1, 2] and dst.integrals.step.tolist() == [2]


# ---- warm start -----------------------------------------------------------------------------------------------------------------
def reader(f):
    from gapflow_amd.io import read_yaml_input
    return read_yaml_input(f)


@pytest.mark.parametrize('eps', [0.7, 0.5])
def test_warm_start_from_the_converged_coarse_run(hiplib, eps):
    """1-D journal bearing: Nx = 50 converged -> init_from -> Nx = 100 run().  It converges, passes the reference's Sommerfeld
    criterion (2 %), its rho agrees with the run from the uniform field to the run's own tol, 1e-8 relative (the CPU oracle gives
    9e-11), and it takes at most 0.75 of that run's steps (the oracle's ratios: 0.46 at eps 0.7, 0.45 at eps 0.5)."""
    from gapflow_amd import Problem

    def from_text(text):
        d = reader(io.StringIO(text))
        d['geometry']['eps'] = eps
        return Problem._from_dict(d)
    coarse = from_text(JOURNAL_1D_COARSE)
    quiet(coarse.run)
    assert coarse.converged and coarse.step < coarse.max_it
    cold = from_text(JOURNAL_1D)
    quiet(cold.run)
    assert cold.converged and cold.step < cold.max_it

    def make(d):
        p = Problem._from_dict(d)
        p.init_from(coarse)
        return p
    warm = quiet(rs.check_sommerfeld, make, reader, eps)
    rho_w, rho_c = np.array(warm.q[0]), np.array(cold.q[0])
    diff = (np.abs(rho_w - rho_c) / np.abs(rho_c)).max()
    print(f"\n[warm start eps {eps}] coarse {coarse.step} steps, fine from uniform {cold.step}, fine from resampled coarse {warm.step} "
          f"(ratio {warm.step / cold.step:.3f}); max relative difference of rho {diff:.2e}")
    assert warm.converged and warm.step < warm.max_it
    assert diff <= 1e-8
    assert warm.step <= 0.75 * cold.step


# ---- from a file, from the command line ---------------------------------------------------------------------------------------
RUN = """
options: {{output: {out}, use_tstamp: False, write_freq: 10, silent: False}}
grid: {{Nx: 30, Ny: 25, Lx: 1.e-3, Ly: 8.e-4, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: asperity, hmin: 4.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, dt: 1.e-10, max_it: 25}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007, P0: 101325., C1: 3.5e10, C2: 1.23}}
"""


def test_from_a_checkpoint_file_and_from_the_command_line(hiplib, tmp_path):
    from gapflow_amd import Problem
    from gapflow_amd.__main__ import main
    src = source(PERIODIC, (12, 10))
    path = str(tmp_path / 'coarse' / 'checkpoint.gpf')
    os.makedirs(os.path.dirname(path))
    src.save_checkpoint(path)
    by_problem, by_path = build(text_of(PERIODIC, (30, 25))), build(text_of(PERIODIC, (30, 25)))
    by_problem.init_from(src)
    by_path.init_from(path)
    assert_bitwise(by_path.q, by_problem.q, 'from the file against from the problem')
    # options.init_from, relative to the YAML file
    (tmp_path / 'yaml.yaml').write_text(text_of(PERIODIC, (30, 25)).replace('silent: True', 'silent: True, init_from: coarse/checkpoint.gpf'))
    by_yaml = quiet(Problem.from_yaml, str(tmp_path / 'yaml.yaml'))
    assert_bitwise(by_yaml.q, by_problem.q, 'options.init_from')
    for name in ('api', 'cli'):
        (tmp_path / f'{name}.yaml').write_text(RUN.format(out=tmp_path / name))
    api = quiet(Problem.from_yaml, str(tmp_path / 'api.yaml'))
    api.init_from(path)
    quiet(api.run)
    assert quiet(main, ['-i', str(tmp_path / 'cli.yaml'), '--init-from', path]) == 0
    hist = [(tmp_path / name / 'history.csv').read_bytes() for name in ('api', 'cli')]
    assert hist[0] == hist[1] and len(hist[0].splitlines()) == 5      # header, steps 0, 10, 20, 25
    # a run from the uniform field writes another history
    (tmp_path / 'plain.yaml').write_text(RUN.format(out=tmp_path / 'plain'))
    assert quiet(main, ['-i', str(tmp_path / 'plain.yaml')]) == 0
    assert (tmp_path / 'plain' / 'history.csv').read_bytes() != hist[0]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def refused(lib, dst, src, code, match):
    from gapflow_amd import _lib
    before, sc = dst._download(_lib.FIELD_Q, 3), scalars_of(dst)     # (the device's field, not the host's mirror)
    rcode = lib.gpf_resample(dst._h, src._h)
    msg = lib.gpf_last_error().decode()
    assert rcode == code, f"{rcode}: {msg}"
    assert 'gpf_resample' in msg and match in msg, msg
    assert_bitwise(dst._download(_lib.FIELD_Q, 3), before, f'dst after the refusal ({match})')
    assert scalars_of(dst) == sc


def test_refusals_through_the_c_abi(hiplib):
    from gapflow_amd import _lib, Ensemble
    lib = _lib.load()
    INVALID, STATE = -1, -5
    src = source(PERIODIC, (12, 10))
    dst = advance(build(text_of(PERIODIC, (30, 25))), 2)
    assert lib.gpf_resample(None, src._h) == INVALID and 'null handle' in lib.gpf_last_error().decode()
    assert lib.gpf_resample(dst._h, None) == INVALID and 'null handle' in lib.gpf_last_error().decode()
    refused(lib, dst, dst, INVALID, 'same handle')
    # geometry
    longer = build(text_of(PERIODIC.replace('Lx: 1.e-3', 'Lx: 1.00001e-3'), (12, 10)))
    refused(lib, dst, longer, INVALID, 'Lx')
    wider = build(text_of(PERIODIC.replace('Ly: 8.e-4', 'Ly: 8.1e-4'), (12, 10)))
    refused(lib, dst, wider, INVALID, 'Ly')
    walls = build(text_of(SLIDER, (16, 8)))
    refused(lib, dst, walls, INVALID, 'periodic')
    # an open stage-wise step, on either side
    other = advance(build(text_of(PERIODIC, (12, 10))), 1)
    _lib.check(lib.gpf_open_step(other._h))
    refused(lib, dst, other, STATE, 'stage-wise step is open on the source')
    _lib.check(lib.gpf_open_step(dst._h))
    for i in range(2):
        _lib.check(lib.gpf_stage_closures(dst._h))
        _lib.check(lib.gpf_stage_advance(dst._h, i))
    rcode = lib.gpf_resample(dst._h, src._h)
    assert rcode == STATE and 'stage-wise step is open on the destination' in lib.gpf_last_error().decode()
    sc = _lib.GpfScalars()
    _lib.check(lib.gpf_close_step(dst._h, C.byref(sc)))
    dst._absorb([sc])
    # a slab: halo rows instead of ghost rows
    cfg = build(text_of(PERIODIC, (12, 10)))._make_config(0)
    cfg.halo_lo = cfg.halo_hi = 1
    slab = C.c_void_p()
    _lib.check(lib.gpf_create(C.byref(cfg), C.byref(slab)))
    try:
        assert lib.gpf_resample(dst._h, slab) == STATE and 'the source is a slab' in lib.gpf_last_error().decode()
        assert lib.gpf_resample(slab, src._h) == STATE and 'the destination is a slab' in lib.gpf_last_error().decode()
    finally:
        lib.gpf_destroy(slab)
    # no q, no gap yet
    cfg = build(text_of(PERIODIC, (12, 10)))._make_config(0)
    bare = C.c_void_p()
    _lib.check(lib.gpf_create(C.byref(cfg), C.byref(bare)))
    try:
        assert lib.gpf_resample(dst._h, bare) == STATE and 'no q or no gap' in lib.gpf_last_error().decode()
        assert lib.gpf_resample(bare, src._h) == STATE and 'no q or no gap' in lib.gpf_last_error().decode()
    finally:
        lib.gpf_destroy(bare)
    # a source whose last step was rolled back
    bad = advance(build(text_of(PERIODIC, (12, 10))), 1)
    bad.q[0, 3, 3] = np.nan
    quiet(bad.update)
    assert bad._scalars().invalid == 1
    refused(lib, dst, bad, STATE, 'flagged invalid')
    # handles on different devices, where there are two
    if lib.gpf_device_count() >= 2:
        from gapflow_amd import Problem
        far = quiet(Problem.from_string, text_of(PERIODIC, (12, 10)), device=1)
        refused(lib, dst, far, INVALID, 'different devices')
    # a member of a live ensemble; free again once the ensemble is gone
    member = build(text_of(PERIODIC, (12, 10)))
    ens = Ensemble([member])
    refused(lib, member, source(PERIODIC, (30, 25)), STATE, 'live ensemble')
    del ens
    import gc
    gc.collect()
    assert lib.gpf_resample(member._h, source(PERIODIC, (30, 25))._h) == 0, lib.gpf_last_error().decode()


# tests/test_gpu_probes.py: SURROGATE (the pressure and the wall shear stress are Gaussian-process surrogates), and the same film
# with analytic closures on half the cells
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
ANALYTIC = SURROGATE[:SURROGATE.index('gp:')].replace('Nx: 200', 'Nx: 100')


def test_a_surrogate_destination_is_refused(hiplib):
    import warnings
    src = advance(build(ANALYTIC), 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dst = build(SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            dst.init_from(src)
        quiet(dst._pre_run)
        refused(dst._lib, dst, src, -1, 'surrogate')


def test_refusals_of_the_python_layer(hiplib):
    src = source(PERIODIC, (12, 10))
    dst = build(text_of(PERIODIC, (30, 25)))
    before = np.array(dst.q)
    with pytest.raises(ValueError, match='Lx'):
        dst.init_from(build(text_of(PERIODIC.replace('Lx: 1.e-3', 'Lx: 1.00001e-3'), (12, 10))))
    with pytest.raises(ValueError, match='periodic'):
        dst.init_from(build(text_of(SLIDER, (16, 8))))
    with pytest.raises(ValueError, match='own source'):
        dst.init_from(dst)
    with pytest.raises(TypeError):
        dst.init_from(42)
    assert_bitwise(dst.q, before, 'dst after the refusals')
    dst.init_from(src)
