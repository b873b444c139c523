"""The shear-thinning series (set_thinning_series / thinning_series / film_thinning, gpf_thinning_series_*) on the device.

Cases, their initial state and the oracle's side: tests/thinning_series_cases.py (its conditions (a), (b) are held on the CPU by
tests/test_thinning_series_host.py).  Held to a tolerance computed from the oracle alone: every quantity of every recorded step
against math.fsum of the oracle's integrands on a stepped twin's downloaded state.  Held bit for bit: the four tau_* against the
tree sum of the wall-stress planes gpf_update_closures leaves for the committed state; load and the four tau0_* against
film_integrals() of a Newtonian twin holding the same state; eta_sum, rate_sum, the extrema and their cells against the device's
leaf operators (models.pressure, models.viscosity) combined in NumPy; every stride, film_thinning() after each step and the
8-byte loads against every = 1; the run against the run with nothing armed.

The leaf operators take a scalar mu0, so the case with piezo-viscosity (a per-cell mu0) is left out of the leaf-operator test;
its tau_* are held bit for bit against the closure planes like every case's."""
import contextlib
import ctypes as C
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import thinning_series_cases as tc
from test_gpu_probes import SCALARS, assert_bitwise, assert_same_scalars, bits, quiet, scalars_of
from test_gpu_series_order import replay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tc.NAMES
FILM_TAU = ('tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')
# 6 x 131: 66 pairs -- pair 63 (columns 127, 128) is the last lane of the first wave, pair 64 (129, 130) the first of the second,
# pair 65 the half pair of the odd end
PLANT = tc._case(grid="Nx: 6, Ny: 131, Lx: 0.0015, Ly: 0.0262")
PLANT_CELLS = [(1, 5), (6, 5), (3, 1), (3, 131), (3, 128), (3, 129)]
ELASTIC = tc._case(grid="Nx: 48, Ny: 30, Lx: 0.05, Ly: 0.03", bc="xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']") + \
    "    elastic: {E: 50e09, v: 0.3, alpha_underrelax: 0.05}\n"


def build_text(text, amp=0., slip=False, pre_run=True):
    from gapflow_amd import Problem
    from gapflow_amd.io import read_yaml_input
    with io.StringIO(text) as f:
        d = read_yaml_input(f)
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'],
                    extra_field=tc.slip_field(d['grid']) if slip else None)
    if amp:
        tc.modulate(p.q, amp)
    if pre_run:
        p._pre_run()
    return p


def build(name):
    text, _, amp, slip = tc.CASES[name]
    return build_text(text, amp, slip)


def flat(rec, k=None):
    get = (lambda n: rec[n]) if isinstance(rec, dict) else (lambda n: getattr(rec, n)[k])
    return np.array([float(get(n)) for n in NAMES])


def cells_of(rec):
    return [list(rec[n + '_cell']) for n in tc.EXTREMA]


def record_run(name, every=1, arm=True):
    """The case's steps with the series armed at `every` (or nothing armed): the series, film_thinning() and q after every step."""
    p = build(name)
    if arm:
        p.set_thinning_series(every)
    out = dict(now=[], now_cells=[], q=[], step=[], time=[])
    for _ in range(tc.CASES[name][1]):
        p.update()
        rec = p.film_thinning()
        out['now'].append(flat(rec))
        out['now_cells'].append(cells_of(rec))
        out['q'].append(p.q.copy())
        out['step'].append(p.step)
        out['time'].append(p.simtime)
    out['scalars'] = scalars_of(p)
    if arm:
        s = p.thinning_series
        out.update(steps=s.step.tolist(), series_time=s.time.copy(), series=np.array([flat(s, k) for k in range(len(s.step))]).reshape(-1, len(NAMES)),
                   cells=s.cells.copy())
    return out, p


@functools.lru_cache(maxsize=None)
def runs(name):
    """Per case, computed once and only read: every = 1, every = 2, nothing armed; the every = 1 problem itself."""
    one, p = record_run(name, 1)
    two, _ = record_run(name, 2)
    plain, _ = record_run(name, arm=False)
    return dict(one=one, two=two, plain=plain, problem=p)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tc.CASE_NAMES)
def test_values_match_the_oracle_sums(hiplib, name):
    """Every quantity of every recorded step against the oracle on the unarmed twin's downloaded state: the sums within
    (1e-12 + n eps) sum|term| dA + 2 x the conditioning allowance of fsum of the integrands, the extrema within the per-cell bound
    of the oracle's per-cell value at the recorded cell and of the oracle's own extremum, their cells the argmin / argmax wherever the
    runner-up is farther away than that bound; step and time equal the twin's in every bit.  Each figure is printed as error /
    tolerance before it is asserted.

    Largest |device - oracle| / tolerance measured on an MI355X, over all steps of a case:
        case                    load     tau_*    tau0_*   eta_sum  rate_sum  eta_min  eta_max  rate_max
        eyring-48x10            6.2e-5   5.9e-4   4.8e-5   6.3e-4   1.0e-3    1.9e-2   6.3e-2   2.2e-2
        carreau-16x1            8.3e-5   9.8e-3   2.1e-4   8.9e-3   5.2e-3    7.2e-3   2.9e-2   1.4e-2
        eyring-roelands-6x601   5.2e-5   9.8e-5   3.5e-4   7.9e-5   1.8e-5    3.7e-4   9.9e-4   3.8e-4
        eyring-24x300-px        5.7e-5   1.7e-4   8.4e-5   1.1e-4   1.2e-4    1.4e-2   1.7e-2   1.4e-2
        eyring-slip-16x41       4.7e-5   1.5e-3   1.2e-4   1.3e-3   9.2e-4    2.8e-2   7.5e-3   3.0e-2
        eyring-mt-20x13         1.9e-4   1.1e-3   1.7e-4   2.5e-4   1.8e-4    1.4e-4   1.5e-2   2.0e-4
    Where the tolerance does NOT hold, and why the cases avoid it: under the stiff Dowson-Higginson law (C1 = 3.5e10) a wave about
    the ambient density (p within a few MPa of zero at its steepest flank) put rate_max at 1.1 to 2.1 and eta_min at 1.4 times
    the per-cell bound (6 x 601 with that law; 16 x 41), the sums still below 0.1.  The cause is not the kernel: the device's
    eos_pressure forms s = rho * (1 / rho0) where the oracle divides, one rounding of s is 2e-5 Pa of p under that law whatever p
    is, and a relative 1e-12 of a small p does not cover it -- the oracle with s formed the device's way, on the CPU, lands at 2
    to 5 bounds in the same states (thinning_series_cases.py; condition (c) of the host test keeps the cases clear of them)."""
    r = runs(name)
    one, plain, p = r['one'], r['plain'], r['problem']
    n = tc.CASES[name][1]
    assert one['steps'] == plain['step'] == list(range(1, n + 1))
    assert_bitwise(one['series_time'], plain['time'], 'time')
    topo, Ls = np.array(p.topo.full[:3]), np.array(p._extra[0])
    worst, bad = {}, {}
    for k in range(n):
        ref = tc.oracle_record(plain['q'][k], topo, Ls, p.prop, p.geo, p.grid)
        got = dict(zip(NAMES, one['series'][k]))
        for q in tc.SUMS:
            w = abs(got[q] - ref['value'][q]) / ref['tol'][q]
            worst[q] = max(worst.get(q, 0.), w)
            if not w <= 1.0:
                bad[(k + 1, q)] = w
        for j, (q, field, pick) in enumerate((('eta_min', 'eta', np.argmin), ('eta_max', 'eta', np.argmax), ('rate_max', 'rate', np.argmax))):
            f, bound = ref[field], ref[field + '_bound']
            ix, iy = (int(v) for v in one['cells'][k, j])
            assert 1 <= ix <= f.shape[0] and 1 <= iy <= f.shape[1], (name, k, q, ix, iy)
            at = np.unravel_index(int(pick(f)), f.shape)
            w = max(abs(got[q] - f[ix - 1, iy - 1]) / bound[ix - 1, iy - 1], abs(got[q] - f[at]) / bound[at])
            worst[q] = max(worst.get(q, 0.), w)
            if not w <= 1.0:
                bad[(k + 1, q)] = w
            others = np.delete(f.ravel(), int(pick(f)))
            if others.size and np.min(np.abs(others - f[at])) > 2. * bound.max():
                assert (ix - 1, iy - 1) == tuple(int(v) for v in at), (name, k + 1, q, (ix, iy), at)
    print(f"\n[{name}] largest |device - oracle| / tolerance: " + ', '.join(f"{q} {w:.3e}" for q, w in worst.items()))
    assert not bad, f"{name}: outside the tolerance (step, quantity): error / tolerance {bad}"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bit for bit against the device's own closures
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tc.CASE_NAMES)
def test_tau_is_the_tree_sum_of_the_closure_planes(hiplib, name):
    """gpf_update_closures runs k_fields_thinning on the committed q: the interior of its wall-stress planes, summed in NumPy in the
    documented tree (tests/test_gpu_series_order.py: replay), is film_thinning()'s tau_* in every bit."""
    p = runs(name)['problem']
    rec = p.film_thinning()
    p._closures_stale = True
    dA = p.grid['dx'] * p.grid['dy']
    xz, yz = p.wall_stress_xz, p.wall_stress_yz
    planes = dict(tau_xz_bot=xz.lower[4], tau_yz_bot=yz.lower[3], tau_xz_top=xz.upper[4], tau_yz_top=yz.upper[3])
    for n, plane in planes.items():
        want = replay(np.ascontiguousarray(plane[1:-1, 1:-1]), dA)
        assert bits(rec[n]) == bits(want), f"{name}: {n} {rec[n]!r} against the tree sum of the closure plane {want!r}"
    assert_bitwise(flat(rec), runs(name)['one']['series'][-1], 'film_thinning() again, behind the closure update')


# ---------------------------------------------------------------------------------------------------------------------------
# 3. bit for bit against the Newtonian twin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tc.CASE_NAMES)
def test_load_and_tau0_are_the_newtonian_twins_film_integrals(hiplib, name):
    text, _, _, slip = tc.CASES[name]
    lines = [ln for ln in text.splitlines() if 'thinning:' not in ln]
    assert len(lines) == len(text.splitlines()) - 1
    twin = build_text('\n'.join(lines) + '\n', 0., slip)
    one = runs(name)['one']
    twin.q[...] = one['q'][-1]
    film = twin.film_integrals()
    got = dict(zip(NAMES, one['series'][-1]))
    assert bits(got['load']) == bits(film['load']), (name, 'load', got['load'], film['load'])
    for n in FILM_TAU:
        assert bits(got[n.replace('tau_', 'tau0_')]) == bits(film[n]), (name, n, got[n.replace('tau_', 'tau0_')], film[n])
        assert bits(got[n]) != bits(film[n]), f"{name}: {n} does not feel the thinning"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. eta_sum, rate_sum, the extrema and their cells from the device's leaf operators
# ---------------------------------------------------------------------------------------------------------------------------
def leaf_record(p, q):
    """name -> value for eta_sum, rate_sum and the extrema, and the extrema's cells: the device's leaf operators on the ghosted
    planes, the differences, the divisions by 2 dx / 2 dy and mu0 factor in NumPy (exactly rounded operations), the documented tree
    and the tie rule (np.argmin / np.argmax over the C-ordered interior: the smaller ix, then the smaller iy)."""
    from gapflow_amd.models import pressure as mp, viscosity as mv
    prop = tc.full_prop(p.prop)
    assert 'piezo' not in prop
    dx, dy, dA = p.grid['dx'], p.grid['dy'], p.grid['dx'] * p.grid['dy']
    pr = mp.eos_pressure(np.ascontiguousarray(q[0]), prop)
    dpx = (pr[2:, 1:-1] - pr[:-2, 1:-1]) / (2 * dx)
    dpy = (pr[1:-1, 2:] - pr[1:-1, :-2]) / (2 * dy)
    h = np.array(p.topo.full[0])[1:-1, 1:-1]
    mu0 = prop['shear']
    rate = mv.shear_rate_avg(dpx, dpy, h, p.geo['U'], p.geo['V'], mu0)
    eta = mu0 * mv.shear_thinning_factor(rate, mu0, prop['thinning'])
    out = dict(eta_sum=replay(eta, dA), rate_sum=replay(rate, dA))
    cells = []
    for n, f, pick in (('eta_min', eta, np.argmin), ('eta_max', eta, np.argmax), ('rate_max', rate, np.argmax)):
        ix, iy = np.unravel_index(int(pick(f)), f.shape)
        out[n] = f[ix, iy]
        cells.append([int(ix) + 1, int(iy) + 1])
    return out, cells


def assert_leaf(rec, p, q, what):
    want, cells = leaf_record(p, q)
    for n, v in want.items():
        assert bits(rec[n]) == bits(v), f"{what}: {n} {rec[n]!r} against the leaf operators' {v!r}"
    assert cells_of(rec) == cells, f"{what}: cells {cells_of(rec)} against {cells}"


@pytest.mark.parametrize('name', [n for n in tc.CASE_NAMES if 'roelands' not in n])
def test_eta_rate_and_extrema_from_the_leaf_operators(hiplib, name):
    r = runs(name)
    p = r['problem']
    assert_leaf(p.film_thinning(), p, r['one']['q'][-1], name)


def test_planted_steps_and_ties(hiplib):
    """A uniform state ties whole columns (h depends on x alone): the first cell under the tie rule wins.  Then the steepest
    pressure step is planted -- one cell's density raised -- at the first and last interior row, the first and last column (the
    last of an odd Ny), and either side of a wave end; the two neighbours along y of a planted cell see the same step over the
    same gap, so rate_max and eta_min are a tie that the smaller iy wins.  Last, the same value is planted in two cells."""
    p = build_text(PLANT)
    base = p.q.copy()
    rec = p.film_thinning()
    assert_leaf(rec, p, base, 'uniform state')
    assert all(c[1] == 1 for c in cells_of(rec)), cells_of(rec)
    for ix, iy in PLANT_CELLS + [((3, 40), (3, 90))]:
        planted = [(ix, iy)] if isinstance(ix, int) else [ix, iy]
        q = base.copy()
        for cx, cy in planted:
            q[0, cx, cy] *= 1. + 1e-4
        p.q[...] = q
        rec = p.film_thinning()
        assert_leaf(rec, p, q, f"planted at {planted}")
        cx, cy = rec['rate_max_cell']
        assert min(abs(cx - a) + abs(cy - b) for a, b in planted) == 1, (planted, rec['rate_max_cell'])
        assert rec['eta_min_cell'] == rec['rate_max_cell']
        if len(planted) == 2:
            assert abs(cx - planted[0][0]) + abs(cy - planted[0][1]) == 1, 'the first of the two planted cells wins the tie'


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a pure function of the state   6. recording only reads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tc.CASE_NAMES)
def test_series_is_film_thinning_after_every_step_at_every_stride(hiplib, name):
    r = runs(name)
    one, two, plain = r['one'], r['two'], r['plain']
    n = tc.CASES[name][1]
    assert one['cells'].shape == (n, 3, 2)
    assert_bitwise(one['series'], np.array(one['now']), f"{name}: the series against film_thinning() after each step")
    assert one['cells'].tolist() == one['now_cells']
    assert two['steps'] == list(range(2, n + 1, 2))
    assert_bitwise(two['series'], one['series'][1::2], f"{name}: every = 2 against every = 1")
    assert two['cells'].tolist() == one['cells'][1::2].tolist()
    assert_bitwise(two['series_time'], one['series_time'][1::2], f"{name}: times")
    assert_bitwise(np.array(plain['now']), one['series'], f"{name}: film_thinning() of the unarmed run")
    for k in range(n):
        assert_bitwise(one['q'][k], plain['q'][k], f"{name}: q after step {k + 1}, armed against unarmed")
        assert_bitwise(two['q'][k], plain['q'][k], f"{name}: q after step {k + 1}, every = 2 against unarmed")
    assert_same_scalars(one['scalars'], plain['scalars'], f"{name}: final scalars")
    assert np.all(np.isfinite(one['series']))


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import thinning_series_cases as tc
import test_gpu_thinning_series as t
out = {{}}
for name in tc.CASE_NAMES:
    one, _ = t.record_run(name, 1)
    out[name], out[name + '_cells'] = one['series'], one['cells']
np.savez({out!r}, **out)
"""


def test_narrow_loads_give_the_same_bits(hiplib, tmp_path):
    """GPF_FILM_NARROW is read when the buffers are allocated: a fresh child process records every case with the 8-byte loads --
    that it did take them is read from the library's GPF_DEBUG trace -- and leaves the bits of this process's 16-byte loads."""
    out = str(tmp_path / 'narrow.npz')
    cmd = [sys.executable, '-c', CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)]
    res = subprocess.run(cmd, env=dict(os.environ, GPF_DEBUG='1', GPF_FILM_NARROW='1'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr.count('k_thin_partial takes 8-byte pair loads') == len(tc.CASE_NAMES) and 'k_thin_partial takes 16-byte' not in res.stderr
    narrow = np.load(out)
    for name in tc.CASE_NAMES:
        wide = runs(name)['one']
        assert_bitwise(narrow[name], wide['series'], f"{name}: narrow against wide loads")
        assert narrow[name + '_cells'].tolist() == wide['cells'].tolist()


def test_beside_probes_extrema_and_statistics_each_series_holds_what_it_holds_alone(hiplib):
    name = 'eyring-48x10'
    n = tc.CASES[name][1]
    cells = [(0, 0), (1, 1), (24, 5), (48, 10), (49, 11)]
    arm = dict(thin=lambda p: p.set_thinning_series(1), probes=lambda p: p.set_probes(cells, pressure=True), extrema=lambda p: p.set_extrema(1),
               stats=lambda p: p.set_statistics(1, ('p', 'rho'), 0))

    def run(which):
        p = build(name)
        for w in which:
            arm[w](p)
        for _ in range(n):
            p.update()
        return p
    both = run(('thin', 'probes', 'extrema', 'stats'))
    assert_bitwise(np.array([flat(both.thinning_series, k) for k in range(n)]), runs(name)['one']['series'], 'thinning series beside the others')
    alone = run(('probes', 'extrema', 'stats'))
    for f in ('rho', 'jx', 'jy', 'p', 'time'):
        assert_bitwise(getattr(both.probes, f), getattr(alone.probes, f), f"probes {f}")
    from gapflow_amd import _lib
    for f in _lib.EXTREMA_NAMES:
        assert_bitwise(getattr(both.extrema, f), getattr(alone.extrema, f), f"extrema {f}")
    assert both.extrema.cells.tolist() == alone.extrema.cells.tolist()
    sb, sa = both.statistics, alone.statistics
    for k in sa:
        if isinstance(sa[k], np.ndarray) and sa[k].dtype == np.float64:
            assert_bitwise(sb[k], sa[k], f"statistics {k}")
    assert_bitwise(both.q, alone.q, 'q')


def test_rolled_back_step_leaves_no_record(hiplib):
    p = build('eyring-48x10')
    p.set_thinning_series(1)
    for _ in range(2):
        p.update()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p.update)
    assert p._stop and p.step == 2
    assert p.thinning_series.step.tolist() == [1, 2]
    n = C.c_int64(-1)
    assert p._lib.gpf_thinning_series_read(p._h, None, None, 0, None, C.byref(n)) == 0 and n.value == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 7. refusals and lifecycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(hiplib):
    from gapflow_amd import _lib
    from gapflow_amd.slab import SlabProblem
    import test_gpu_probes as tp
    text = tc.CASES['eyring-48x10'][0]
    newton = build_text('\n'.join(ln for ln in text.splitlines() if 'thinning:' not in ln) + '\n')
    lib = newton._lib
    vals, cells = np.zeros(14), np.zeros(6, dtype=np.int32)
    vp, cp = vals.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_int32))
    ms = C.c_double(0.)
    with pytest.raises(NotImplementedError, match='no shear thinning'):
        newton.set_thinning_series(1)
    with pytest.raises(NotImplementedError, match='no shear thinning'):
        newton.film_thinning()
    assert newton.thinning_series is None
    assert lib.gpf_thinning_series_set(newton._h, 1) == -5 and b'no shear thinning' in lib.gpf_last_error()
    assert lib.gpf_thinning_series_now(newton._h, vp, cp) == -5 and b'no shear thinning' in lib.gpf_last_error()
    assert lib.gpf_thinning_series_time(newton._h, 1, 0, C.byref(ms)) == -5 and b'no shear thinning' in lib.gpf_last_error()
    assert lib.gpf_thinning_series_read(newton._h, None, None, 0, None, None) == -5 and b'not armed' in lib.gpf_last_error()
    assert lib.gpf_thinning_series_set(None, 1) == -1
    with pytest.raises(NotImplementedError, match='thinning series: not available on a SlabProblem'):
        SlabProblem.set_thinning_series(object(), 1)
    # a slab handle: halo rows on one side
    p = build('eyring-48x10')
    cfg = p._make_config(0)
    cfg.halo_lo = 1
    slab = C.c_void_p()
    _lib.check(lib.gpf_create(C.byref(cfg), C.byref(slab)))
    try:
        assert lib.gpf_thinning_series_set(slab, 1) == -5 and b'slab' in lib.gpf_last_error()
    finally:
        lib.gpf_destroy(slab)
    # a surrogate problem: at the Python level (the host test holds the message) and at the C ABI
    sur = tp.build(tp.SURROGATE.replace('EOS: BWR,', 'EOS: BWR, thinning: {name: Eyring, tauE: 5.e4},'))
    assert sur._cfg.thinning and sur._gp_models
    with pytest.raises(NotImplementedError, match='surrogates'):
        sur.set_thinning_series(1)
    with pytest.raises(NotImplementedError, match='surrogates'):
        sur.film_thinning()
    assert lib.gpf_thinning_series_set(sur._h, 1) == -1 and b'surrogate closures' in lib.gpf_last_error()
    assert lib.gpf_thinning_series_now(sur._h, vp, cp) == -1 and b'surrogate closures' in lib.gpf_last_error()
    # an open step
    with pytest.raises(ValueError, match='thinning series'):
        p.set_thinning_series(0)
    assert lib.gpf_thinning_series_set(p._h, 0) == -1 and b'every >= 1' in lib.gpf_last_error()
    _lib.check(lib.gpf_open_step(p._h))
    assert lib.gpf_thinning_series_set(p._h, 1) == -5 and b'open' in lib.gpf_last_error()
    assert lib.gpf_thinning_series_now(p._h, vp, cp) == -5 and b'open' in lib.gpf_last_error()
    for stage in range(2):
        _lib.check(lib.gpf_stage_closures(p._h))
        _lib.check(lib.gpf_stage_advance(p._h, stage))
    _lib.check(lib.gpf_close_step(p._h, None))
    assert lib.gpf_thinning_series_set(p._h, 2) == 0
    assert lib.gpf_thinning_series_clear(p._h) == 0


def test_clear_rearm_and_pre_run_start_a_new_series(hiplib):
    p = build('eyring-48x10')
    p.set_thinning_series(1)
    for _ in range(3):
        p.update()
    assert p.thinning_series.step.tolist() == [1, 2, 3]
    p.clear_thinning_series()
    p.update()
    assert p.thinning_series is None and p.step == 4
    p.set_thinning_series(2)
    assert p.thinning_series.step.shape == (0,) and p.thinning_series.cells.shape == (0, 3, 2)
    for _ in range(3):
        p.update()
    assert p.thinning_series.step.tolist() == [6]
    p._pre_run()
    assert p.thinning_series.step.shape == (0,)
    p.update()
    p.update()
    assert p.thinning_series.step.tolist() == [2]


def test_time_entry_point_steps_and_records(hiplib):
    """gpf_thinning_series_time: n stage-wise steps inside the library; mode 1 leaves the records of the armed stride, bit for bit
    those of update(); mode 0 leaves none and the same state."""
    name = 'eyring-48x10'
    n = tc.CASES[name][1]
    p = build(name)
    p.set_thinning_series(1)
    ms = C.c_double(-1.)
    from gapflow_amd import _lib
    _lib.check(p._lib.gpf_thinning_series_time(p._h, n, 1, C.byref(ms)))
    assert ms.value > 0.
    vals, steps, have = np.zeros((n, 14)), np.zeros(n, dtype=np.int64), C.c_int64(0)
    _lib.check(p._lib.gpf_thinning_series_read(p._h, _lib.as_dp(vals), None, n, steps.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(have)))
    assert have.value == n and steps.tolist() == list(range(1, n + 1))
    assert_bitwise(vals, runs(name)['one']['series'], 'mode 1 against update()')
    q = build(name)
    q.set_thinning_series(1)
    _lib.check(q._lib.gpf_thinning_series_time(q._h, n, 0, C.byref(ms)))
    _lib.check(q._lib.gpf_thinning_series_read(q._h, None, None, 0, None, C.byref(have)))
    assert have.value == 0


def test_run_writes_the_file_and_a_restored_problem_rearms(hiplib, tmp_path):
    from gapflow_amd import Problem
    text = tc.CASES['eyring-48x10'][0].replace('silent: True', f"silent: False, output: {tmp_path / 'run'}, write_freq: 5, use_tstamp: False, thinning_series: 2")
    text = text.replace('max_it: 100', 'max_it: 8')
    assert 'thinning_series: 2' in text and 'max_it: 8' in text
    p = quiet(Problem.from_string, text)
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'thinning_series.npz'))
    assert sorted(f.files) == sorted(('step', 'time', 'cells') + NAMES)
    assert f['step'].tolist() == [2, 4, 6, 8] and f['cells'].shape == (4, 3, 2)
    rec = p.film_thinning()
    for n in NAMES:
        assert bits(f[n][-1]) == bits(rec[n]), n
    p.save_checkpoint(str(tmp_path / 'c.gpf'))
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'), options={'silent': True})
    assert b.thinning_series is not None and b.thinning_series.step.shape == (0,)
    b.update()
    b.update()
    assert b.thinning_series.step.tolist() == [10]


def test_with_an_elastic_gap_the_record_follows_the_deformed_gap(hiplib):
    """Thinning and an elastic gap combine: the record waits for the deformation that follows the step and equals film_thinning()
    of the state and the DEFORMED gap the problem then holds, in every bit; it is not the record of the gap before the update."""
    p = build_text(ELASTIC, 2e-5)
    p.set_thinning_series(1)
    before, now = [], []
    for _ in range(4):
        gap = np.array(p.topo.full[:3])
        p.update()
        now.append(flat(p.film_thinning()))
        rigid = build_text(ELASTIC.replace("    elastic: {E: 50e09, v: 0.3, alpha_underrelax: 0.05}\n", ''), 0.)
        rigid.q[...] = p.q
        rigid.topo.full[:3] = gap
        rigid._upload_topo()
        before.append(flat(rigid.film_thinning()))
    s = p.thinning_series
    assert s.step.tolist() == [1, 2, 3, 4]
    got = np.array([flat(s, k) for k in range(4)])
    assert_bitwise(got, np.array(now), 'the series against film_thinning() behind each deformation')
    assert np.abs(np.array(p.topo.full[3])).max() > 0., 'the gap did deform'
    assert not np.array_equal(bits(got[-1]), bits(before[-1])), 'the record is the one of the gap before the deformation'
