"""Field extrema (gpf_extrema_*, Problem.set_extrema / extrema / field_extrema) on the device, against the state itself.

The reference of every value is the downloaded state: NumPy's max / min over the interior cells of q and of the gap, with
np.argmax / np.argmin over the C-ordered interior, whose first occurrence is the record's tie rule (smallest ix, then smallest
iy).  rho, h and |j / rho| are compared BITWISE -- the operands are the same and both divisions are IEEE (the bitwise form was
sufficient; the fall-back of comparing the value at the recorded cell was not needed).  p is compared bitwise against probes
with pressure=True at every interior cell on the 1-D problem; on the 2-D problems against gapflow_amd.models.pressure at
rtol 1e-12, the tolerance tests/test_gpu_probes.py holds the probes' p to, with the cells exact."""
import contextlib
import ctypes as C
import functools
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import reference_suite as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('p_max', 'p_min', 'rho_max', 'rho_min', 'h_min', 'u_max', 'v_max')
SCALARS = ('step', 'simtime', 'dt', 'ekin', 'ekin_old', 'residual', 'v_max', 'v_sound', 'mass', 'invalid', 'converged')
P_RTOL = 1e-12

# the reference's Sommerfeld test: 1-D periodic Dowson-Higginson journal bearing, Nx = 100 (one workgroup: k_small_steps)
JOURNAL_1D = rs.JOURNAL_1D


def journal_2d(nx, ny):
    """The same bearing on nx x ny cells, periodic in both directions, the same length in x (k_step2 beyond 1200 ghosted cells)."""
    return JOURNAL_1D.replace("dx: 1.e-5", f"dx: {1.e-3 / nx!r}").replace("dy: 1.\n", "dy: 1.e-5\n") \
        .replace("Nx: 100", f"Nx: {nx}").replace("Ny: 1\n", f"Ny: {ny}\n").replace("C1: 3.5e12", "C1: 3.5e10")


# a flat gap and a uniform state: every cell ties with every other
FLAT = """
options: {{silent: True}}
grid: {{dx: 1.e-5, dy: 1.e-5, Nx: {nx}, Ny: {ny}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: inclined, hmin: 5.e-6, hmax: 5.e-6, U: 0.1, V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-8, dt: 1e-10, max_it: 1000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""

# tests/test_gpu_extras.py: THINNING, its 1-D Eyring case (stage-wise steps)
THINNING_1D = """
options: {silent: True}
grid: {Nx: 48, Ny: 1, Lx: 0.05, Ly: 1., xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: parabolic, hmin: 1.e-5, hmax: 4.e-5, U: 10., V: 0.}
numerics: {CFL: 0.4, adaptive: 1, max_it: 100}
properties:
    EOS: DH
    shear: 0.05
    bulk: 0.
    rho0: 877.7007
    thinning: {name: Eyring, tauE: 5.e5}
"""

# tests/test_gpu_elastic.py: BASE with its 'periodic_2d' case (48 x 30, the gap deforms after every step)
ELASTIC = """
options: {silent: True}
grid: {Lx: 0.0762, Ly: 0.04, Nx: 48, Ny: 30}
geometry: {type: parabolic, hmin: 2.54e-5, hmax: 5.08e-5, U: 4.57, V: 0.3}
numerics: {adaptive: 1, CFL: 0.45, tol: 1e-8, dt: 1.e-10, max_it: 60}
properties:
    EOS: Bayada
    rho0: 850.
    shear: 0.039
    bulk: 0.
    cl: 1600.
    cv: 352.
    elastic: {E: 50e09, v: 0.3, alpha_underrelax: 0.05}
    piezo: {name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}
"""


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


def scalars_of(p):
    sc = p._scalars()
    return tuple(getattr(sc, k) for k in SCALARS)


def first_extreme(field, want_min):
    """(value, (ix, iy)) of the interior field [Nx][Ny]: np.argmax's first occurrence in C order is the record's tie rule."""
    k = int(np.argmin(field) if want_min else np.argmax(field))
    ix, iy = divmod(k, field.shape[1])
    return field[ix, iy], (ix + 1, iy + 1)


def occurrences(field, want_min):
    best = field.min() if want_min else field.max()
    return np.count_nonzero(field == best)


def is_unique(field, want_min):
    return occurrences(field, want_min) == 1


def state_fields(q, h):
    """The five interior fields the record is taken of, without p: rho, rho, h, |jx / rho|, |jy / rho| in the record's order."""
    rho, jx, jy = (q[c, 1:-1, 1:-1] for c in range(3))
    return {'rho_max': rho, 'rho_min': rho, 'h_min': h[1:-1, 1:-1], 'u_max': np.abs(jx / rho), 'v_max': np.abs(jy / rho)}


def want_min(name):
    return name.endswith('_min')


def assert_record_is_the_states(rec, cells, q, h, what, p_field=None, prop=None, need_unique=False, check_p=True, known_ties=None):
    """rec: {name: value}, cells: {name: (ix, iy)} against the downloaded q and gap.  p_field: the interior pressure to hold p_*
    to bitwise (probes); otherwise prop: models.pressure of the downloaded density at P_RTOL, cells exact.  check_p=False: the
    1-D problem's law is stiff (C1 = 3.5e12) and its p is held bitwise to the probes' in the first test, not to models.pressure."""
    fields = state_fields(q, h)
    for name, f in fields.items():
        if need_unique and not np.all(f == f.flat[0]):          # (a field that is one value everywhere ties in every cell: (1, 1))
            assert occurrences(f, want_min(name)) == (known_ties or {}).get(name, 1), f"{what}: {name} is not unique on the host: the comparison could pass by luck"
        v, cell = first_extreme(f, want_min(name))
        assert bits(rec[name]) == bits(v), f"{what}: {name} {rec[name]!r} on the device, {v!r} from the state"
        assert tuple(cells[name]) == cell, f"{what}: {name} at {tuple(cells[name])} on the device, {cell} from the state"
    if not check_p:
        return
    if p_field is None:
        from gapflow_amd.models.pressure import eos_pressure
        p_field = eos_pressure(fields['rho_max'], prop)
    for name in ('p_max', 'p_min'):
        v, cell = first_extreme(p_field, want_min(name))
        if prop is None:
            if need_unique:
                assert is_unique(p_field, want_min(name)), f"{what}: {name} is not unique on the host"
            assert bits(rec[name]) == bits(v), f"{what}: {name} {rec[name]!r} on the device, {v!r} from the probes"
        else:
            # cells within the tolerance of the extreme must hold the extreme's own density (exact ties, which both sides break
            # alike): otherwise the rounding of p could decide the cell
            near = np.abs(p_field - v) <= 4. * P_RTOL * abs(v)
            assert np.all(bits(fields['rho_max'][near]) == bits(fields['rho_max'][cell[0] - 1, cell[1] - 1])), f"{what}: {name}: near-ties on the host"
            np.testing.assert_allclose(rec[name], v, rtol=P_RTOL, atol=0., err_msg=f"{what}: {name}")
        assert tuple(cells[name]) == cell, f"{what}: {name} at {tuple(cells[name])} on the device, {cell} expected"


def series_record(s, k):
    return {n: getattr(s, n)[k] for n in NAMES}, {n: tuple(int(c) for c in s.cells[k, s.index[n]]) for n in NAMES}


def now_record(p):
    r = p.field_extrema()
    return {n: r[n] for n in NAMES}, {n: r[n + '_cell'] for n in NAMES}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the small kernel, against the state itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_small_kernel_series_is_the_stepped_twins_extrema(hiplib):
    """One batch of 40 steps with every = 1 inside k_small_steps against a twin that takes 40 single steps and downloads q and
    the gap after each; p from a probe with pressure=True at each of the 100 interior cells of the twin, bitwise.
    Every extremum is asserted unique on the host at every step, with two exceptions that no eps removes: jy is zero in every
    cell of this 1-D problem (V = 0), so v_max ties everywhere and belongs to (1, 1); and the journal's gap is a cosine sampled
    at the cell centres of an even Nx, mirror-symmetric about its minimum, so cells 50 and 51 hold the same bits and h_min
    belongs to (50, 1).  The host asserts exactly those ties (two occurrences, no more), which makes h_min a check of the
    tie rule on a real field: a device that kept (51, 1) fails."""
    n = 40
    p, twin = build(JOURNAL_1D), build(JOURNAL_1D)
    p.set_extrema(1)
    p._advance(n, honor_stop=False)
    s = p.extrema
    assert s.step.tolist() == list(range(1, n + 1)) and s.cells.shape == (n, 7, 2) and s.p_max.shape == (n,)
    assert s.index == {name: k for k, name in enumerate(NAMES)}
    twin.set_probes([(ix, 1) for ix in range(1, 101)], pressure=True)
    for k in range(n):
        twin.update()
        rec, cells = series_record(s, k)
        assert bits(s.time[k]) == bits(twin.simtime)
        assert_record_is_the_states(rec, cells, twin.q, twin.topo.h, f"step {k + 1}", p_field=twin.probes.p[k].reshape(100, 1), need_unique=True,
                                    known_ties={'h_min': 2})
    assert_bitwise(p.q, twin.q, 'final q, batch against single steps')
    rec, cells = now_record(p)
    assert (rec, cells) == series_record(s, n - 1), 'field_extrema() of the final state against the last record'


# ---------------------------------------------------------------------------------------------------------------------------
# 2. launch-per-step path, ragged shapes, wide against narrow loads
# ---------------------------------------------------------------------------------------------------------------------------
RAGGED = {'37x71': (37, 71), '300x5': (300, 5)}


@functools.lru_cache(maxsize=None)
def ragged_run(name):
    """Six recorded steps in one call; computed once per shape and only read by the tests."""
    p = build(journal_2d(*RAGGED[name]))
    p.set_extrema(1)
    p._advance(6, honor_stop=False)
    s = p.extrema
    return dict(values=np.array([getattr(s, n) for n in NAMES]).T.copy(), cells=s.cells.copy(), step=s.step.copy(), time=s.time.copy())


@pytest.mark.parametrize('name', sorted(RAGGED))
def test_two_launch_series_is_the_stepped_twins_extrema(hiplib, name):
    """37 x 71: odd Ny, the last pair reaches the ghost column.  300 x 5: the fold's second trip, idle threads in a row."""
    run = ragged_run(name)
    twin = build(journal_2d(*RAGGED[name]))
    assert run['step'].tolist() == [1, 2, 3, 4, 5, 6]
    for k in range(6):
        twin.update()
        rec = dict(zip(NAMES, run['values'][k]))
        cells = {n: tuple(int(c) for c in run['cells'][k, i]) for i, n in enumerate(NAMES)}
        assert bits(run['time'][k]) == bits(twin.simtime)
        assert_record_is_the_states(rec, cells, twin.q, twin.topo.h, f"{name} step {k + 1}", prop=twin.prop)


CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import test_gpu_extrema as t
out = {{}}
for name in sorted(t.RAGGED):
    r = t.ragged_run(name)
    out[name + '_values'], out[name + '_cells'] = r['values'], r['cells']
np.savez({out!r}, **out)
"""


def test_narrow_loads_give_the_same_bits(hiplib, tmp_path):
    """GPF_FILM_NARROW is read when the buffers are allocated: a fresh child process records both shapes with the 8-byte loads.
    That it did take them is read from the library's GPF_DEBUG trace of that allocation, once per shape; the same child without
    the variable reports the 16-byte loads, so the comparison is not of the wide path with itself."""
    out = str(tmp_path / 'narrow.npz')
    cmd = [sys.executable, '-c', CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)]
    env = {k: v for k, v in os.environ.items() if k != 'GPF_FILM_NARROW'}
    res = subprocess.run(cmd, env=dict(env, GPF_DEBUG='1'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr.count('k_extrema_partial takes 16-byte pair loads') == len(RAGGED) and '8-byte pair loads' not in res.stderr
    assert_bitwise(np.load(out)['37x71_values'], ragged_run('37x71')['values'], 'a child process against this one')
    res = subprocess.run(cmd, env=dict(env, GPF_DEBUG='1', GPF_FILM_NARROW='1'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr.count('k_extrema_partial takes 8-byte pair loads') == len(RAGGED) and '16-byte pair loads' not in res.stderr
    narrow = np.load(out)
    for name in sorted(RAGGED):
        wide = ragged_run(name)
        assert_bitwise(narrow[name + '_values'], wide['values'], f"{name}: narrow against wide loads")
        assert narrow[name + '_cells'].tolist() == wide['cells'].tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ties
# ---------------------------------------------------------------------------------------------------------------------------
# Tied cells planted into the flat state, per shape a list of (cells of the maxima, cells of the minima), chosen so that a tie
# crosses every boundary of the shared fold (csrc/series_first.hpp).  A row's workgroup gives thread t the column pairs
# (1 + 2k, 2 + 2k), k = t, t + 256, ...; lanes fold inside a wave of 64, thread 0 folds the waves, and the fold kernel gives thread
# t the rows t, t + 256, ...:
#   3 x 5      3 pairs: one partly filled wave
#   5 x 130    65 pairs: columns 128 | 129 are lane 63 of wave 0 and lane 0 of wave 1
#   2 x 515    258 pairs, the pair loop wraps: columns 513, 514 are thread 0's second pair, columns 3, 4 thread 1's first -- the
#              lower thread holds the later cell; column 515 shares its pair with the ghost column
#   258 x 4    the row loop wraps: row 257 is thread 0's second, row 2 thread 1's first
TIED = {
    (12, 9): [([(5, 9), (5, 2), (11, 1)], [(12, 9), (3, 3), (3, 8)])],
    (40, 70): [([(20, 66), (20, 65), (39, 1)], [(7, 70), (7, 1), (40, 2)])],
    (3, 5): [([(2, 5), (2, 3), (3, 1)], [(1, 5), (1, 4), (3, 2)]), ([(3, 5), (3, 4)], [(3, 1), (2, 2)])],
    (5, 130): [([(3, 129), (3, 128), (5, 1)], [(2, 130), (2, 129), (4, 64)]), ([(4, 130), (4, 127)], [(1, 129), (1, 128)])],
    (2, 515): [([(1, 513), (1, 4), (2, 1)], [(2, 515), (2, 512), (2, 3)]), ([(1, 513), (1, 512)], [(2, 515), (2, 514)]),
               ([(2, 514), (2, 259)], [(1, 515), (1, 258), (1, 257)])],
    (258, 4): [([(257, 1), (2, 3), (258, 1)], [(257, 4), (258, 2), (3, 1)]), ([(257, 1), (256, 4)], [(257, 2), (1, 4)]),
               ([(258, 4), (258, 3)], [(130, 2), (129, 3)])],
}


@pytest.mark.parametrize('nx,ny', list(TIED), ids=['small-kernel-size', 'two-launch-size'] + [f'{nx}x{ny}' for nx, ny in list(TIED)[2:]])
def test_ties_go_to_the_first_cell(hiplib, nx, ny):
    """The flat gap under the uniform state ties in every cell: every record belongs to (1, 1).  Then the tied sets of TIED,
    written into p.q and topo.h before the first step: rho (so p_max, rho_max) and jy (v_max) raised in the cells of the maxima,
    rho (p_min, rho_min, and u_max through |jx / rho|) and h (h_min) lowered in the cells of the minima, to one value each.  The
    expectation is NumPy's first hit in the row-major interior of the planted arrays; the library is not asked."""
    p = build(FLAT.format(nx=nx, ny=ny))
    q, h = p.q, p.topo.h
    for f in state_fields(q, h).values():
        assert np.all(bits(f) == bits(f[0, 0])), 'the flat gap and the uniform state tie in every cell'
    r = p.field_extrema()
    for name in NAMES:
        assert r[name + '_cell'] == (1, 1), name
    assert bits(r['rho_max']) == bits(q[0, 1, 1]) and bits(r['h_min']) == bits(h[1, 1]) and bits(r['u_max']) == bits(abs(q[1, 1, 1] / q[0, 1, 1]))
    q0, h0 = q.copy(), h.copy()
    assert q0[0, 1, 1] > 0. and q0[1, 1, 1] != 0. and h0[1, 1] > 0.
    for hi, lo in TIED[(nx, ny)]:
        assert not set(hi) & set(lo) and all(1 <= ix <= nx and 1 <= iy <= ny for ix, iy in hi + lo)
        q, hp = p.q, h0.copy()
        q[...] = q0
        for ix, iy in hi:
            q[0, ix, iy] = (1. + 2. ** -10) * q0[0, 1, 1]
            q[2, ix, iy] = 1e-3
        for ix, iy in lo:
            q[0, ix, iy] = (1. - 2. ** -10) * q0[0, 1, 1]
            hp[ix, iy] = 0.5 * h0[1, 1]
        p.topo.h = hp
        rec, cells = now_record(p)
        first_hi, first_lo = min(hi), min(lo)           # the row-major first of each set ...
        assert first_hi != hi[0] and first_lo != lo[0], 'the sets list a later cell first'
        what = f"{nx} x {ny}, ties at {hi} and {lo}"
        assert_record_is_the_states(rec, cells, p.q, p.topo.h, what, prop=p.prop)
        # ... which is what NumPy found, and every quantity has its tie (no comparison above passed on a unique cell)
        for name in NAMES:
            assert cells[name] == (first_lo if name in ('p_min', 'rho_min', 'h_min', 'u_max') else first_hi), f"{what}: {name} at {cells[name]}"
        for name, f in state_fields(p.q, p.topo.h).items():
            assert occurrences(f, want_min(name)) == len(lo if name in ('rho_min', 'h_min', 'u_max') else hi), f"{what}: {name} does not tie"


# ---------------------------------------------------------------------------------------------------------------------------
# 3b. a single extreme at every position
# ---------------------------------------------------------------------------------------------------------------------------
PLANT_PARTS = 2


@pytest.mark.parametrize('nx,ny,part', [(nx, ny, k) for nx, ny in ((5, 130), (258, 4)) for k in range(PLANT_PARTS)],
                         ids=lambda v: str(v))
def test_planted_extreme_is_found_at_every_position(hiplib, nx, ny, part):
    """One strict maximum of rho and one strict minimum of h, planted into the flat state at every interior cell in turn (rho at
    the cell, h at its point mirror, so that the two walk the grid in opposite directions), one field_extrema() per plant: the
    values and the cells are the planted ones, whichever thread, lane, wave and trip of the shared fold holds them.  5 x 130: 65
    pairs, two waves in a row's workgroup.  258 x 4: the fold's row loop wraps.  The positions are dealt to PLANT_PARTS cases."""
    p = build(FLAT.format(nx=nx, ny=ny))
    q0, h0 = p.q.copy(), p.topo.h.copy()
    rho_up, h_down = (1. + 2. ** -10) * q0[0, 1, 1], 0.5 * h0[1, 1]
    positions = [(ix, iy) for ix in range(1, nx + 1) for iy in range(1, ny + 1)][part::PLANT_PARTS]
    for ix, iy in positions:
        mx, my = nx + 1 - ix, ny + 1 - iy
        q, hp = p.q, h0.copy()
        q[...] = q0
        q[0, ix, iy] = rho_up
        hp[mx, my] = h_down
        p.topo.h = hp
        r = p.field_extrema()
        assert r['rho_max_cell'] == (ix, iy) and bits(r['rho_max']) == bits(rho_up), f"rho_max planted at {(ix, iy)}: {r['rho_max']!r} at {r['rho_max_cell']}"
        assert r['p_max_cell'] == (ix, iy), f"p_max with rho_max planted at {(ix, iy)}: at {r['p_max_cell']}"
        assert r['h_min_cell'] == (mx, my) and bits(r['h_min']) == bits(h_down), f"h_min planted at {(mx, my)}: {r['h_min']!r} at {r['h_min_cell']}"
        assert r['rho_min_cell'] == ((1, 1) if (ix, iy) != (1, 1) else (1, 2) if ny > 1 else (2, 1)), 'the cells left flat tie: the first of them'
    assert len(positions) >= nx * ny // PLANT_PARTS


# ---------------------------------------------------------------------------------------------------------------------------
# 4. batching and stride
# ---------------------------------------------------------------------------------------------------------------------------
def series_of(text, batches, every):
    p = build(text)
    p.set_extrema(every)
    for n in batches:
        p._advance(n, honor_stop=False)
    s = p.extrema
    return s.step.tolist(), np.array([s.time] + [getattr(s, n) for n in NAMES]), s.cells.tolist()


@pytest.mark.parametrize('text', [JOURNAL_1D, journal_2d(37, 71)], ids=['small-1d', '37x71'])
def test_series_does_not_depend_on_the_batches(hiplib, text):
    one = series_of(text, [10], 3)
    assert one[0] == [3, 6, 9]
    for batches in ([1] * 10, [4, 6]):
        other = series_of(text, batches, 3)
        assert other[0] == [3, 6, 9] and other[2] == one[2]
        assert_bitwise(other[1], one[1], f"batches {batches} against one batch of 10")


def test_small_batch_is_not_cut(hiplib):
    """The library exposes no launch counter, so: gpf_extrema_time at n = 2000, mode 1 (every = 1) against mode 0, alternating,
    the smallest of three each.  A batch cut at every record is 2000 launches of k_small_steps, each of which costs a launch
    (5 us at the very least on this runtime, csrc/small_kernel.hip) and reloads the field; one batch with the records written
    inside it costs one launch and a workgroup fold per step.  Bound: less than 2.5 us per step added, half the cheapest launch."""
    n = 2000
    p = build(JOURNAL_1D)
    p.set_extrema(1)
    p._advance(8, honor_stop=False)
    ms = C.c_double(0.)
    t = {0: [], 1: []}
    for _ in range(3):
        for mode in (0, 1):
            assert p._lib.gpf_extrema_time(p._h, n, mode, C.byref(ms)) == 0, p._lib.gpf_last_error()
            t[mode].append(ms.value)
    off, on = min(t[0]), min(t[1])
    print(f"\n[extrema, Nx = 100 small kernel, n = {n}] unarmed {off / n * 1e3:.3f} us/step, armed at every = 1 {on / n * 1e3:.3f} us/step, "
          f"ratio {on / off:.3f}, added {(on - off) / n * 1e3:.3f} us/step")
    assert (on - off) / n * 1e3 < 2.5, f"armed {on:.3f} ms against {off:.3f} ms for {n} steps: the batch looks cut"
    have = C.c_int64(0)
    assert p._lib.gpf_extrema_read(p._h, None, None, 0, None, C.byref(have)) == 0 and have.value == n


# ---------------------------------------------------------------------------------------------------------------------------
# 5. recording only reads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('text,cells', [(JOURNAL_1D, [(1, 1), (50, 1), (100, 1)]), (journal_2d(37, 71), [(1, 1), (20, 36), (37, 71)])],
                         ids=['small-1d', '37x71'])
def test_recording_leaves_the_run_unchanged(hiplib, text, cells):
    armed, plain = build(text), build(text)
    armed.set_probes(cells, pressure=True)
    plain.set_probes(cells, pressure=True)
    armed.set_extrema(1)
    la = armed._advance(30, honor_stop=False)
    lp = plain._advance(30, honor_stop=False)
    assert_bitwise(armed.q, plain.q, 'q after 30 steps, with and without extrema')
    for a, b in zip(la, lp):
        for k in SCALARS:
            x, y = getattr(a, k), getattr(b, k)
            assert (bits(x) == bits(y)) if isinstance(x, float) else x == y, f"scalar history: {k} {x!r} vs {y!r}"
    for x, y in zip(scalars_of(armed), scalars_of(plain)):
        assert (bits(x) == bits(y)) if isinstance(x, float) else x == y
    for name in ('rho', 'jx', 'jy', 'p'):
        assert_bitwise(getattr(armed.probes, name), getattr(plain.probes, name), f"probes alongside: {name}")
    assert armed.extrema.step.tolist() == list(range(1, 31))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. stop and rollback
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('text', [JOURNAL_1D, journal_2d(37, 71)], ids=['small-1d', '37x71'])
def test_rolled_back_batch_leaves_the_records_before_it(hiplib, text):
    """tests/test_gpu_parity.py: test_invalid_state_rolls_back's way to an invalid state (an absurd time step), under honor_stop:
    the batch rolls back at step 4, the series holds steps 1..3, and the invalid run state has no extrema to give."""
    p = build(text)
    p.set_extrema(1)
    p._advance(3, honor_stop=True)
    good, h = p.q.copy(), p.topo.h.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=True)
    assert p._stop and p.step == 3
    np.testing.assert_array_equal(p.q, good)
    s = p.extrema
    assert s.step.tolist() == [1, 2, 3] and s.cells.shape == (3, 7, 2)
    rec, cells = series_record(s, 2)
    assert_record_is_the_states(rec, cells, good, h, 'last record against the state the rollback kept', prop=p.prop, check_p=p.grid['Ny'] > 1)
    vals, cl = np.zeros(7), np.zeros(14, dtype=np.int32)
    assert p._lib.gpf_extrema_now(p._h, vals.ctypes.data_as(C.POINTER(C.c_double)), cl.ctypes.data_as(C.POINTER(C.c_int32))) == -5      # GPF_ERR_STATE
    assert b'invalid' in p._lib.gpf_last_error()


@pytest.mark.parametrize('text', [JOURNAL_1D, journal_2d(37, 71)], ids=['small-1d', '37x71'])
def test_batch_that_commits_steps_and_then_rolls_back(hiplib, text):
    """A rollback in the middle of ONE batch: a fixed step size beyond the stable one lets the explicit scheme grow until a
    density turns negative, an ordinary invalid state some tens of steps in.  The batch then holds committed, recorded steps
    and, behind them, the rolled-back step and the steps that never ran.  The series must hold exactly the multiples of the
    stride up to the last committed step, and its last record must be that of the matching single-stepped twin.
    (On the launch-per-step path the kernels queued behind the rollback are told step counts the device never reaches and
    must write nothing; the slots they would write lie beyond what the host collects, so the ABI cannot show them.)"""
    n, every = 400, 5
    dt = build(text).dt
    for factor in (2., 3., 5., 8., 16.):
        fixed = text.replace('adaptive: 1', 'adaptive: 0').replace('dt: 1e-10', f'dt: {factor * dt!r}')
        p = build(fixed)
        p.set_extrema(every)
        quiet(p._advance, n, honor_stop=True)
        print(f"\n[rollback inside a batch] dt = {factor} x the CFL step: {p.step} of {n} steps committed, stopped: {p._stop}")
        if p._stop and every <= p.step < n:
            break
    assert p._stop and every <= p.step < n, 'no step size gave a rollback inside the batch'
    k = p.step
    s = p.extrema
    assert s.step.tolist() == list(range(every, k + 1, every))
    twin = build(fixed)
    last = s.step[-1]
    twin._advance(int(last), honor_stop=False)
    rec, cells = series_record(s, len(s.step) - 1)
    assert_record_is_the_states(rec, cells, twin.q, twin.topo.h, f"record of step {last}, before the rollback at step {k + 1}", check_p=False)
    assert bits(s.time[-1]) == bits(twin.simtime)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. stage-wise problems
# ---------------------------------------------------------------------------------------------------------------------------
def test_shear_thinning_problem_records_a_series(hiplib):
    p = build(THINNING_1D)
    p.set_extrema(2)
    for k in range(6):
        p.update()
        if p.step % 2 == 0:
            rec, cells = series_record(p.extrema, p.step // 2 - 1)
            assert_record_is_the_states(rec, cells, p.q, p.topo.h, f"thinning step {p.step}", prop=p.prop)
    assert p.extrema.step.tolist() == [2, 4, 6]


def test_elastic_problem_records_the_deformed_gap(hiplib):
    """h_min of every record is the minimum of the deformed gap downloaded after that step, bitwise, with its cell."""
    p = build(ELASTIC)
    p.set_extrema(1)
    h0 = p.topo.h.copy()
    for k in range(5):
        p.update()
        s = p.extrema
        assert s.step.tolist() == list(range(1, k + 2))
        h = p.topo.h
        v, cell = first_extreme(h[1:-1, 1:-1], True)
        assert bits(s.h_min[k]) == bits(v) and tuple(s.cells[k, s.index['h_min']]) == cell
        for name, f in state_fields(p.q, h).items():
            fv, fcell = first_extreme(f, want_min(name))
            assert bits(getattr(s, name)[k]) == bits(fv) and tuple(s.cells[k, s.index[name]]) == fcell, name
    assert not np.array_equal(p.topo.h, h0), 'the gap did deform'
    assert bits(p.field_extrema()['h_min']) == bits(p.extrema.h_min[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# 8. refusals and lifecycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_surrogate_pressure_is_refused(hiplib):
    """tests/test_gpu_probes.py: SURROGATE (pressure and shear from Gaussian processes): the class set_probes(pressure=True) raises."""
    from gapflow_amd import Problem
    import test_gpu_probes as tp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p = quiet(Problem.from_string, tp.SURROGATE)
        with pytest.raises(ValueError, match='surrogate'):
            p.set_extrema(1)
        with pytest.raises(ValueError, match='surrogate'):
            p.field_extrema()
        quiet(p._pre_run)
        assert p._lib.gpf_extrema_set(p._h, 1) == -1 and b'surrogate' in p._lib.gpf_last_error()
    assert p.extrema is None


def test_library_refusals_and_clear(hiplib):
    p = build(JOURNAL_1D)
    assert p._lib.gpf_extrema_set(None, 1) == -1
    assert p._lib.gpf_extrema_set(p._h, 0) == -1 and b'every >= 1' in p._lib.gpf_last_error()
    assert p._lib.gpf_extrema_read(p._h, None, None, 0, None, None) == -5           # not armed
    with pytest.raises(ValueError, match='extrema'):
        p.set_extrema(0)
    assert p.extrema is None
    p.set_extrema(1)
    p._advance(3, honor_stop=False)
    assert p.extrema.step.tolist() == [1, 2, 3]
    p.clear_extrema()
    p._advance(3, honor_stop=False)
    assert p.extrema is None and p.step == 6
    p.set_extrema(2)                        # a new series
    assert p.extrema.step.shape == (0,) and p.extrema.cells.shape == (0, 7, 2)
    p._advance(3, honor_stop=False)
    assert p.extrema.step.tolist() == [8]


def run_yaml(out, silent, max_it=12):
    options = f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, extrema: 2}}"
    return JOURNAL_1D.replace("options:\n    output: data/journal\n    write_freq: 1000\n    silent: True\n", options + "\n") \
        .replace('max_it: 10_000', f'max_it: {max_it}')


def test_run_writes_extrema_npz(hiplib, tmp_path):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'extrema.npz'))
    assert sorted(f.files) == sorted(('step', 'time', 'cells', 'names') + NAMES)
    assert f['step'].tolist() == [2, 4, 6, 8, 10, 12] and f['cells'].shape == (6, 7, 2) and f['names'].tolist() == list(NAMES)
    rec = {n: f[n][-1] for n in NAMES}
    cells = {n: tuple(int(c) for c in f['cells'][-1, k]) for k, n in enumerate(NAMES)}
    assert_record_is_the_states(rec, cells, p.q, p.topo.h, 'last record of the run against q', check_p=False)


def test_restored_problem_rearms_and_starts_a_new_series(hiplib, tmp_path):
    """Checkpoints do not carry the series: the restored problem's begins after the restart step."""
    from gapflow_amd import Problem
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(4, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.extrema is not None and b.extrema.step.shape == (0,)
    b._advance(4, honor_stop=False)
    assert a.extrema.step.tolist() == [2, 4, 6, 8] and b.extrema.step.tolist() == [6, 8]
    for name in ('time',) + NAMES:
        assert_bitwise(getattr(b.extrema, name), getattr(a.extrema, name)[2:], name)
    assert b.extrema.cells.tolist() == a.extrema.cells[2:].tolist()


def test_ensemble_refuses_an_armed_member_and_takes_it_cleared(hiplib):
    from gapflow_amd import Ensemble
    texts = [JOURNAL_1D, JOURNAL_1D.replace('eps: 0.7', 'eps: 0.5')]
    members, alone = [build(t) for t in texts], [build(t) for t in texts]
    members[1].set_extrema(1)
    with pytest.raises(NotImplementedError, match='member 1: extrema are armed'):
        Ensemble(members)
    handles = (C.c_void_p * 2)(*[m._h.value for m in members])
    e = C.c_void_p()
    assert members[0]._lib.gpf_ensemble_create(handles, 2, C.byref(e)) == -1
    assert b'member 1: extrema are armed on it' in members[0]._lib.gpf_last_error()
    members[1].clear_extrema()
    ens = Ensemble(members)
    ens.step(7)
    for m, a in zip(members, alone):
        a._advance(7, honor_stop=False)
        assert_bitwise(m.q, a.q, 'member against the problem alone')
    got = ens.field_extrema()
    assert [r['p_max_cell'] for r in got] == [a.field_extrema()['p_max_cell'] for a in alone]
    assert all(bits(r['p_max']) == bits(a.field_extrema()['p_max']) for r, a in zip(got, alone))
