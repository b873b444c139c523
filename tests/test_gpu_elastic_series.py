"""An elastic Problem's film integrals (set_integrals / integrals / film_integrals) and its deformation series
(set_elastic_series / elastic_series / film_elastic, gpf_elastic_series_*) on the device.

Both are recorded behind gpf_elastic_update, with the state, the gap and the deformation the handle then holds.  Held bit for
bit: a series' record against the `_now` record taken after that same update(), every stride against every = 1, the 8-byte
against the 16-byte loads, the run's q against the run with nothing armed, and the film integrals against a RIGID problem that is
given the elastic run's state and deformed gap.  Held to a tolerance: the deformation series' sums against math.fsum of the
NumPy terms on the downloaded planes (test_values_match_numpy_on_the_downloaded_planes).

Shapes: tests/test_gpu_elastic.py's 'periodic_2d' (48 x 30, the gap deforms every step) restated, 48 x 31 (the last pair of a
row reaches the ghost column), 260 x 6 (a fold thread adds two rows) and its 'free_2d' (a non-periodic half-space, 48 x 30).

Not covered: a rolled-back step followed by a committed one.  The project's recipe for an invalid step (gpf_set_dt with an
absurd step, tests/test_gpu_parity.py) leaves the run state invalid, and the stage-wise path has no way back from that:
gpf_open_step refuses.  test_rolled_back_step_leaves_no_record holds the first half."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEP = 12
SUMS = ('d_sum', 'd2_sum', 'p_d', 'h_sum')
NAMES = SUMS + ('d_max', 'd_min')
FILM = ('load', 'load_x', 'load_y', 'p_hx', 'p_hy', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')

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
{elastic}    piezo: {{name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}}
"""
ELASTIC = "    elastic: {E: 50e09, v: 0.3, alpha_underrelax: 0.05}\n"
DN = "xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 850., xW_D: 850., yS: ['D', 'N', 'N'], yN: ['D', 'N', 'N'], yS_D: 850., yN_D: 850."
GRIDS = {
    '48x30': "Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 30",
    '48x31': "Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 31",
    '260x6': "Lx: 0.0762, Ly: 0.04, Nx: 260, Ny: 6",
    '6x150': "Lx: 0.009525, Ly: 0.2, Nx: 6, Ny: 150",           # the cells of 48x30; 75 column pairs: two waves, the second partly filled
    'free-48x30': f"Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 30, {DN}",
}
SHAPES = sorted(GRIDS)


def text_of(name, elastic=True, options=''):
    return BASE.format(grid=GRIDS[name], elastic=ELASTIC if elastic else '', options=options)


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


def film_flat(rec, k=None):
    """The film integrals' record as one vector: the nine sums, flow_x, flow_y (of record k of a series, or of a `_now` dict)."""
    get = (lambda n: rec[n]) if isinstance(rec, dict) else (lambda n: getattr(rec, n)[k])
    return np.concatenate([[get(n) for n in FILM], np.ravel(get('flow_x')), np.ravel(get('flow_y'))])


def record_run(name, every=1, arm=True):
    """NSTEP update() calls with both series armed at `every` (or nothing armed): the series, and behind every update the `_now`
    records of the state the problem then holds."""
    p = build(text_of(name))
    if arm:
        p.set_integrals(every)
        p.set_elastic_series(every)
    now_film, now_el = [], []
    for _ in range(NSTEP):
        p.update()
        now_film.append(film_flat(p.film_integrals()))
        now_el.append(p.film_elastic())
    out = dict(q=p.q.copy(), now_film=np.array(now_film), now_el=now_el, topo=np.array(p.topo.full), time=p.simtime)
    if arm:
        s, e = p.integrals, p.elastic_series
        out.update(film_steps=s.step.tolist(), film=np.array([film_flat(s, k) for k in range(len(s.step))]), film_time=s.time.copy(),
                   el_steps=e.step.tolist(), el=np.array([[getattr(e, n)[k] for n in NAMES] for k in range(len(e.step))]),
                   el_cells=e.cells.copy(), el_time=e.time.copy())
    return out, p


@functools.lru_cache(maxsize=None)
def runs(name):
    """Per shape, computed once and only read: every = 1, every = 3, nothing armed; the every = 1 problem itself."""
    one, p = record_run(name, 1)
    three, _ = record_run(name, 3)
    plain, _ = record_run(name, arm=False)
    return dict(one=one, three=three, plain=plain, problem=p)


# ---------------------------------------------------------------------------------------------------------------------------
# film integrals of an elastic problem
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SHAPES)
def test_integral_series_is_film_integrals_after_every_update(hiplib, name):
    """(a) every record equals, bit for bit, film_integrals() called after that same update(); a stride keeps its multiples with
    the same bits; the run's q is that of the run with nothing armed."""
    r = runs(name)
    one, three, plain = r['one'], r['three'], r['plain']
    assert one['film_steps'] == list(range(1, NSTEP + 1))
    assert_bitwise(one['film'], one['now_film'], f"{name}: the series against film_integrals() after each update")
    assert three['film_steps'] == [3, 6, 9, 12]
    assert_bitwise(three['film'], one['film'][2::3], f"{name}: every = 3 against every = 1")
    assert_bitwise(three['film_time'], one['film_time'][2::3], f"{name}: times")
    assert_bitwise(one['q'], plain['q'], f"{name}: q with both series armed against q with nothing armed")
    assert_bitwise(three['q'], plain['q'], f"{name}: q at every = 3")
    assert_bitwise(one['topo'], plain['topo'], f"{name}: the deformed gap")
    assert not r['problem'].integrals_in_batch
    assert np.abs(one['topo'][3]).max() > 0., 'the gap did deform'


@pytest.mark.parametrize('name', SHAPES)
def test_record_sees_the_deformed_gap_of_its_state(hiplib, name):
    """(b) a rigid problem of the same input that is handed the elastic run's q and its deformed h, dh/dx, dh/dy returns from
    film_integrals() the elastic problem's last record in every bit: the record pairs the state with the gap of that state, not
    with the gap of the step before and not with the undeformed one."""
    one = runs(name)['one']
    rigid = build(text_of(name, elastic=False))
    undeformed = film_flat(rigid.film_integrals())
    rigid.q[...] = one['q']
    rigid.topo.full[:3] = one['topo'][:3]
    rigid._upload_topo()
    assert_bitwise(film_flat(rigid.film_integrals()), one['film'][-1], f"{name}: a rigid problem on the elastic run's state and gap")
    assert not np.array_equal(bits(undeformed), bits(one['film'][-1]))


def test_rolled_back_step_leaves_no_record(hiplib):
    """(d), its first half: tests/test_gpu_parity.py's way to an invalid state (an absurd time step) on the stage-wise path.  The
    step is rolled back, no series gains a record, and a gpf_elastic_update behind it writes none."""
    p = build(text_of('48x30'))
    p.set_integrals(1)
    p.set_elastic_series(1)
    for _ in range(2):
        p.update()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p.update)
    assert p._stop and p.step == 2
    assert p.integrals.step.tolist() == [1, 2] and p.elastic_series.step.tolist() == [1, 2]
    assert p._lib.gpf_elastic_update(p._h) == 0
    n = C.c_int64(-1)
    assert p._lib.gpf_integrals_read(p._h, None, 0, None, C.byref(n)) == 0 and n.value == 0
    assert p._lib.gpf_elastic_series_read(p._h, None, None, 0, None, C.byref(n)) == 0 and n.value == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the deformation series
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SHAPES)
def test_elastic_series_is_film_elastic_after_every_update(hiplib, name):
    """(e) every record equals, bit for bit, film_elastic() called after that same update(), cells included; a stride keeps its
    multiples with the same bits."""
    r = runs(name)
    one, three = r['one'], r['three']
    assert one['el_steps'] == list(range(1, NSTEP + 1)) and one['el_cells'].shape == (NSTEP, 2, 2)
    now = np.array([[rec[n] for n in NAMES] for rec in one['now_el']])
    assert_bitwise(one['el'], now, f"{name}: the series against film_elastic() after each update")
    assert one['el_cells'].tolist() == [[list(rec['d_max_cell']), list(rec['d_min_cell'])] for rec in one['now_el']]
    assert three['el_steps'] == [3, 6, 9, 12]
    assert_bitwise(three['el'], one['el'][2::3], f"{name}: every = 3 against every = 1")
    assert three['el_cells'].tolist() == one['el_cells'][2::3].tolist()
    assert_bitwise(three['el_time'], one['el_time'][2::3], f"{name}: times")
    assert_bitwise(one['el_time'], one['film_time'], f"{name}: both series' times")


def numpy_record(p, q, topo):
    """name -> (fsum of the terms times dx dy, sum |term| dx dy) for the sums, and the extrema with their cells, from the planes."""
    from gapflow_amd import _lib
    from oracle import closures as ocl
    prop = dict(_lib.EOS_DEFAULTS[p.prop['EOS']], **p.prop)
    rho, h, d = q[0, 1:-1, 1:-1], topo[0, 1:-1, 1:-1], topo[3, 1:-1, 1:-1]
    pr = ocl.eos_pressure(rho, prop)
    dA = p.grid['dx'] * p.grid['dy']
    out = {}
    for n, t in dict(d_sum=d, d2_sum=d * d, p_d=pr * d, h_sum=h).items():
        out[n] = (math.fsum(t.ravel().tolist()) * dA, math.fsum(np.abs(t).ravel().tolist()) * dA)
    for n, k in (('d_max', int(np.argmax(d))), ('d_min', int(np.argmin(d)))):
        ix, iy = divmod(k, d.shape[1])
        out[n] = (d[ix, iy], (ix + 1, iy + 1))
    return out


@pytest.mark.parametrize('name', SHAPES)
def test_values_match_numpy_on_the_downloaded_planes(hiplib, name):
    """(f) the record of the last step against NumPy on the downloaded q, gap and deformation: d_max, d_min and their cells exact
    (np.argmax / np.argmin over the C-ordered interior is the record's tie rule), the sums within 64 * 2^-53 * sum|term| of
    math.fsum of the terms, p from oracle/closures.py.  The bound: a tree at most 24 deep on these shapes (8 + 2 additions per
    row, 8 + 2 + 1 over the rows, fewer than 24), one rounding per product, one for dx dy, and a p at rounding distance from
    NumPy's.  Each figure is printed as error / bound before it is asserted."""
    r = runs(name)
    one, p = r['one'], r['problem']
    ref = numpy_record(p, one['q'], one['topo'])
    got = dict(zip(NAMES, one['el'][-1]))
    u = 2.0 ** -53
    worst = {}
    for n in SUMS:
        val, mag = ref[n]
        worst[n] = abs(got[n] - val) / (64. * u * mag) if mag > 0 else (0. if got[n] == val else np.inf)
    print(f"\n[{name}] |device - fsum| / (64 u sum|term|): " + ', '.join(f"{n} {w:.3e}" for n, w in worst.items()))
    for k, n in enumerate(('d_max', 'd_min')):
        assert bits(got[n]) == bits(ref[n][0]) and tuple(one['el_cells'][-1, k]) == ref[n][1], (name, n, got[n], ref[n], one['el_cells'][-1, k])
    bad = {n: w for n, w in worst.items() if not w <= 1.0}
    assert not bad, f"{name}: outside the bound (error / bound): {bad}"


def test_a_problem_that_has_not_stepped_records_zeros(hiplib):
    """(g) after _pre_run the deformation is +0.0 everywhere: d_sum, d2_sum and p_d are exactly +0.0, d_max = d_min = 0.0, both at
    cell (1, 1) by the tie rule."""
    p = build(text_of('48x31'))
    rec = p.film_elastic()
    for n in ('d_sum', 'd2_sum', 'p_d', 'd_max', 'd_min'):
        assert bits(rec[n]) == bits(0.0), (n, rec[n])
    assert rec['d_max_cell'] == (1, 1) and rec['d_min_cell'] == (1, 1)
    h = p.topo.h[1:-1, 1:-1]
    want = math.fsum(h.ravel().tolist()) * p.grid['dx'] * p.grid['dy']
    assert abs(rec['h_sum'] - want) <= 64. * 2.0 ** -53 * want


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_elastic_series as t
out = {{}}
for name in t.SHAPES:
    one, _ = t.record_run(name, 1)
    out[name + '_film'], out[name + '_el'], out[name + '_cells'] = one['film'], one['el'], one['el_cells']
np.savez({out!r}, **out)
"""


def test_narrow_loads_give_the_same_bits(hiplib, tmp_path):
    """(c), (e) GPF_FILM_NARROW is read when the buffers are allocated: a fresh child process records every shape with the 8-byte
    loads -- that it did take them is read from the library's GPF_DEBUG trace of the allocation -- and leaves the bits of this
    process, which took the 16-byte loads."""
    out = str(tmp_path / 'narrow.npz')
    cmd = [sys.executable, '-c', CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)]
    res = subprocess.run(cmd, env=dict(os.environ, GPF_DEBUG='1', GPF_FILM_NARROW='1'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr.count('k_eldef_partial takes 8-byte pair loads') == len(SHAPES) and 'k_eldef_partial takes 16-byte' not in res.stderr
    narrow = np.load(out)
    for name in SHAPES:
        wide = runs(name)['one']
        assert_bitwise(narrow[name + '_film'], wide['film'], f"{name}: film integrals, narrow against wide loads")
        assert_bitwise(narrow[name + '_el'], wide['el'], f"{name}: deformation series, narrow against wide loads")
        assert narrow[name + '_cells'].tolist() == wide['el_cells'].tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals and lifecycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(hiplib):
    """(h) a rigid problem, a slab handle, an open step: at the Python level and at the C ABI, with codes and message fragments."""
    from gapflow_amd import _lib
    rigid = build(text_of('48x30', elastic=False))
    lib = rigid._lib
    vals, cells = np.zeros(6), np.zeros(4, dtype=np.int32)
    vp, cp = vals.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_int32))
    ms = C.c_double(0.)
    with pytest.raises(NotImplementedError, match='no elastic gap'):
        rigid.set_elastic_series(1)
    with pytest.raises(NotImplementedError, match='no elastic gap'):
        rigid.film_elastic()
    assert rigid.elastic_series is None
    assert lib.gpf_elastic_series_set(rigid._h, 1) == -5 and b'no elastic gap' in lib.gpf_last_error()
    assert lib.gpf_elastic_series_now(rigid._h, vp, cp) == -5 and b'no elastic gap' in lib.gpf_last_error()
    assert lib.gpf_elastic_series_time(rigid._h, 1, 0, C.byref(ms)) == -5 and b'no elastic gap' in lib.gpf_last_error()
    assert lib.gpf_elastic_series_read(rigid._h, None, None, 0, None, None) == -5 and b'not armed' in lib.gpf_last_error()
    assert lib.gpf_elastic_series_set(None, 1) == -1
    # a slab handle: halo rows on one side
    cfg = rigid._make_config(0)
    cfg.halo_lo = 1
    slab = C.c_void_p()
    _lib.check(lib.gpf_create(C.byref(cfg), C.byref(slab)))
    try:
        assert lib.gpf_elastic_series_set(slab, 1) == -5 and b'slab' in lib.gpf_last_error()
        assert lib.gpf_integrals_set(slab, 1, 0, None, 0, None) == -5 and b'slab' in lib.gpf_last_error()
    finally:
        lib.gpf_destroy(slab)
    # an open step
    p = build(text_of('48x30'))
    with pytest.raises(ValueError, match='elastic series'):
        p.set_elastic_series(0)
    assert lib.gpf_elastic_series_set(p._h, 0) == -1 and b'every >= 1' in lib.gpf_last_error()
    _lib.check(lib.gpf_open_step(p._h))
    assert lib.gpf_elastic_series_set(p._h, 1) == -5 and b'open' in lib.gpf_last_error()
    assert lib.gpf_elastic_series_now(p._h, vp, cp) == -5 and b'open' in lib.gpf_last_error()
    assert lib.gpf_integrals_set(p._h, 1, 0, None, 0, None) == -5 and b'open' in lib.gpf_last_error()
    for stage in range(2):
        _lib.check(lib.gpf_stage_closures(p._h))
        _lib.check(lib.gpf_stage_advance(p._h, stage))
    _lib.check(lib.gpf_close_step(p._h, None))
    assert lib.gpf_elastic_series_set(p._h, 2) == 0
    assert lib.gpf_elastic_series_clear(p._h) == 0


def test_clear_and_rearm_start_a_new_series(hiplib):
    p = build(text_of('48x30'))
    p.set_elastic_series(1)
    p.set_extrema(1)            # armed beside another series an elastic problem accepts
    for _ in range(3):
        p.update()
    assert p.elastic_series.step.tolist() == [1, 2, 3] and p.extrema.step.tolist() == [1, 2, 3]
    p.clear_elastic_series()
    p.update()
    assert p.elastic_series is None and p.step == 4
    p.set_elastic_series(2)
    assert p.elastic_series.step.shape == (0,) and p.elastic_series.cells.shape == (0, 2, 2)
    for _ in range(3):
        p.update()
    assert p.elastic_series.step.tolist() == [6]
    assert bits(p.elastic_series.h_sum[0]) != bits(0.0)


def test_run_writes_both_files_and_a_restored_problem_rearms(hiplib, tmp_path):
    """A non-silent run() writes integrals.npz and elastic_series.npz; checkpoints do not carry the series, the options re-arm
    them."""
    from gapflow_amd import Problem
    opts = f", output: {tmp_path / 'run'}, write_freq: 5, use_tstamp: False, integrals: 2, elastic_series: 3"
    text = text_of('48x30', options=opts).replace('silent: True', 'silent: False').replace('max_it: 60', 'max_it: 12')
    p = quiet(Problem.from_string, text)
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'elastic_series.npz'))
    assert sorted(f.files) == sorted(('step', 'time', 'cells') + NAMES)
    assert f['step'].tolist() == [3, 6, 9, 12] and f['cells'].shape == (4, 2, 2)
    rec = p.film_elastic()
    for n in NAMES:
        assert bits(f[n][-1]) == bits(rec[n]), n
    g = np.load(os.path.join(p.outdir, 'integrals.npz'))
    assert g['step'].tolist() == [2, 4, 6, 8, 10, 12]
    assert bits(g['load'][-1]) == bits(p.film_integrals()['load'])
    p.save_checkpoint(str(tmp_path / 'c.gpf'))
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'), options={'silent': True})
    assert b.elastic_series is not None and b.elastic_series.step.shape == (0,) and b.integrals.step.shape == (0,)
