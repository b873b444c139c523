"""Weighted film integrals (gpf_weighted_*, Problem.set_weighted_integrals / weighted_integrals / film_weighted,
options.weighted_integrals + options.weights): sum w_k f dA for up to 8 weight planes and nine integrands, reduced on the device
while gpf_step advances whole batches.

Inputs: the cases of tests/test_gpu_integrals.py (Ny = 1, 300, 601 -- odd, more than one column pair per thread --, a slip-length
field, the row-coefficient and the planes topographies).  Yardsticks:
  * a plane of ones against Problem.integrals of a twin, bit for bit (p against load, the four tau_*): with the product w * f
    rounded on its own, 1.0 adds f's bits in k_film_partial's order;
  * math.fsum of the oracle's integrands (oracle/closures.py) times the weights on the stepped twin's state, tolerance
    (1e-12 + n eps) fsum|w f| dA with n the interior cells -- test_values_match_the_oracle_sums' rule: 1e-12 is the per-cell
    tolerance the project holds cell_fields and the device EOS to, n eps bounds the rounding of any summation order, and the one
    more rounding of w * f per cell (eps) disappears in it;
  * everything else bit for bit: a record is a pure function of the state and the planes, and recording only reads.
Reference: none (post-processing there)."""
import ctypes as C
import functools
import math
import os
import warnings

import numpy as np
import pytest

import test_gpu_probes as tp
from test_gpu_integrals import CASES, PIEZO_WIDE, SLIP_FIELD, STRIDED, build
from test_gpu_probes import (JOURNAL_1D, SCALARS, SLIDER_2D, SURROGATE, THINNING, assert_bitwise, assert_same_scalars, bits, quiet,
                             scalars_of)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
NAMES = list(CASES)
INTEGRANDS = ('p', 'h', 'rho_h', 'jx_h', 'jy_h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')
PLANES = ('ones', 'row_lo', 'row_hi', 'col_lo', 'col_hi', 'cos', 'sin', 'random')
assert PIEZO_WIDE and STRIDED and SLIP_FIELD           # (the inputs behind CASES['piezo-wide' / 'strided-pairs' / 'slip-field'])

# tests/test_gpu_extrema.py: ELASTIC (48 x 30, the gap deforms after every step), restated
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


def split(grid):
    """(row r, column c): the boxes rows 1..r | r+1..Nx and columns 1..c | c+1..Ny partition the interior.  c is odd, the lower
    column of a thread's pair (c, c + 1), so the column boxes cut a pair in the middle; Ny = 1 has no column to cut at (None)."""
    nx, ny = grid['Nx'], grid['Ny']
    r = max(1, nx // 2 - 1)
    c = None if ny < 2 else (ny // 2) | 1
    if c is not None and c >= ny:
        c = 1
    return r, c


def planes_of(p):
    """The K = 8 planes of PLANES for the problem's grid: ones, the two row boxes, the two column boxes (Ny = 1: the first and the
    last interior cell, one-cell boxes), one cos and one sin mode (sign-changing), a smooth random plane from a fixed seed."""
    from gapflow_amd import weights
    g = p.grid
    nx, ny = g['Nx'], g['Ny']
    r, c = split(g)
    rows = [weights.box(g, 1, r, 1, ny), weights.box(g, r + 1, nx, 1, ny)]
    cols = [weights.box(g, 1, nx, 1, c), weights.box(g, 1, nx, c + 1, ny)] if c is not None else \
        [weights.box(g, 1, 1, 1, 1), weights.box(g, nx, nx, 1, 1)]
    rng = np.random.default_rng(20240611)
    smooth = np.zeros((nx, ny))
    for kx in range(3):
        for ky in range(3 if ny > 1 else 1):
            a, b = rng.standard_normal(2)
            smooth += a * weights.mode(g, kx, ky, 'cos') + b * weights.mode(g, kx, ky, 'sin')
    return np.stack([np.ones((nx, ny))] + rows + cols + [weights.mode(g, 2, 1 if ny > 1 else 0, 'cos'), weights.mode(g, 1, 0, 'sin'), smooth])


def oracle_terms(p):
    """(9, Nx, Ny): the oracle's integrands of the problem's current state on the interior cells, in INTEGRANDS' order."""
    from gapflow_amd import _lib
    from oracle import closures as ocl
    q, topo, Ls = np.array(p.q), np.array(p.topo.full[:3]), np.array(p._extra[0])
    prop = dict(_lib.EOS_DEFAULTS[p.prop['EOS']], **p.prop)
    U, V, zeta = p.geo['U'], p.geo['V'], p.prop['bulk']
    pr = ocl.eos_pressure(q[0], prop)
    eta = ocl.piezoviscosity(pr, p.prop['shear'], p.prop['piezo']) if 'piezo' in p.prop else p.prop['shear']
    bot = ocl.stress_bottom(q, topo, U, V, eta, zeta, Ls, slip="top")
    top = ocl.stress_top(q, topo, U, V, eta, zeta, Ls, slip="top")
    terms = [pr, topo[0], q[0] * topo[0], q[1] * topo[0], q[2] * topo[0], bot[4], bot[3], top[4], top[3]]
    return np.stack([np.broadcast_to(t, q[0].shape)[1:-1, 1:-1] for t in terms])


def oracle_sums(terms, planes, dA):
    """(value, tolerance), each (K, 9): fsum of w f over the interior times dA, and (1e-12 + n eps) fsum|w f| dA."""
    val, tol = np.empty((len(planes), len(terms))), np.empty((len(planes), len(terms)))
    for k, w in enumerate(planes):
        for j, t in enumerate(terms):
            wt = (w * t).ravel()
            val[k, j] = math.fsum(wt) * dA
            tol[k, j] = (1e-12 + wt.size * EPS) * math.fsum(np.abs(wt)) * dA
    return val, tol


def armed(name, every=1, planes=None):
    p = build(name)
    p.set_weighted_integrals(planes_of(p) if planes is None else planes, every, PLANES if planes is None else None)
    return p


def series_arrays(s):
    return [(n, getattr(s, n)) for n in ('time',) + INTEGRANDS]


def assert_same_series(a, b, what, pick=None):
    """Bitwise; `pick`: indices of a's records to hold against all of b's."""
    sel = (lambda v: v[pick]) if pick is not None else (lambda v: v)
    assert sel(a.step).tolist() == b.step.tolist(), what
    assert a.names == b.names
    for (n, x), (_, y) in zip(series_arrays(a), series_arrays(b)):
        assert_bitwise(sel(x), y, f"{what}: {n}")


@functools.lru_cache(maxsize=None)
def case_runs(name):
    """One recorded batch (every = 1, the 8 planes); a twin advanced by single update() calls with the same planes and the film
    integrals armed (its two series, its film_weighted() and the oracle's integrands after every step); the same batch with
    nothing armed.  Computed once per case and only read by the tests."""
    _, n, _, sx, sy = CASES[name]
    rec, twin, plain = armed(name), armed(name), build(name)
    twin.set_integrals(1, sx, sy)
    log = rec._advance(n, honor_stop=False)
    plain_log = plain._advance(n, honor_stop=False)
    steps, terms, now = [], [], []
    for _ in range(n):
        twin.update()
        steps.append(twin.step)
        terms.append(oracle_terms(twin))
        now.append(twin.film_weighted())
    return dict(series=rec.weighted_integrals, q=rec.q.copy(), scalars=scalars_of(rec), log=[tuple(getattr(e, k) for k in SCALARS) for e in log],
                plain_q=plain.q.copy(), plain_scalars=scalars_of(plain), plain_log=[tuple(getattr(e, k) for k in SCALARS) for e in plain_log],
                twin_series=twin.weighted_integrals, twin_integrals=twin.integrals, twin_steps=steps, terms=terms, now=now,
                twin_q=twin.q.copy(), planes=planes_of(rec), dA=rec.grid['dx'] * rec.grid['dy'], grid=dict(rec.grid))


PAIRS = (('p', 'load'), ('tau_xz_bot', 'tau_xz_bot'), ('tau_yz_bot', 'tau_yz_bot'), ('tau_xz_top', 'tau_xz_top'), ('tau_yz_top', 'tau_yz_top'))


@pytest.mark.parametrize('name', NAMES)
def test_ones_reproduce_the_film_integrals_bit_for_bit(hiplib, name):
    """w = 1: p and the four tau_* of plane 0 against load and the tau_* of Problem.integrals on the twin, every recorded step."""
    r = case_runs(name)
    s, f, n = r['series'], r['twin_integrals'], CASES[name][1]
    assert s.names == PLANES and s.step.tolist() == f.step.tolist() == list(range(1, n + 1))
    assert s.p.shape == (n, 8)
    assert_bitwise(s.time, f.time, 'time')
    for mine, theirs in PAIRS:
        assert_bitwise(getattr(s, mine)[:, 0], getattr(f, theirs), f"ones: {mine} against the integrals' {theirs}")


@pytest.mark.parametrize('name', ['strided-pairs', 'slip-field', 'small-1d'])
def test_ones_reproduce_the_film_integrals_with_narrow_loads(hiplib, name, monkeypatch):
    """GPF_FILM_NARROW (read by gpf_weighted_set): the 8-byte loads -- an odd Ny walked in strides (the half pair at the end), a
    slip-length field (the eighth plane read), Ny = 1 (nothing but a half pair) -- give the wide loads' series in every bit."""
    r = case_runs(name)                             # wide loads: computed before the variable is set, or by an earlier test
    n = CASES[name][1]
    monkeypatch.setenv('GPF_FILM_NARROW', '1')
    p = armed(name)
    p._advance(n, honor_stop=False)
    assert_same_series(p.weighted_integrals, r['series'], '8-byte loads against 16-byte loads')
    for mine, theirs in PAIRS:
        assert_bitwise(getattr(p.weighted_integrals, mine)[:, 0], getattr(r['twin_integrals'], theirs), f"narrow ones: {mine}")
    now = p.film_weighted()
    for q in INTEGRANDS:
        assert_bitwise(now[q], getattr(r['series'], q)[n - 1], f"film_weighted() with 8-byte loads: {q}")


@pytest.mark.parametrize('name', NAMES)
def test_boxes_select(hiplib, name):
    """The row boxes and the column boxes (cut at an odd column: in the middle of a thread's pair) each within the tolerance of
    the oracle, and each pair of boxes sums to the ones plane's record within both tolerances: no cell lost, none counted twice.
    A box of one cell equals that cell's term times dx dy EXACTLY, all nine integrands: h, rho h, jx h, jy h against the host's
    own product (one rounding each); the wall stresses against components 4 and 3 of the derived fields WALL_LOWER / WALL_UPPER that
    a second problem evaluates on the same state (k_fields: the same cell_fields<EOS>, another kernel); p against the derived
    field PRESSURE, except for Dowson-Higginson, where the integrals' pressure is film_pressure and not eos_pressure (DESIGN
    3.3f) and the yardstick is the oracle's pressure, whose bits film_pressure reproduces (tests/test_integrals_host.py).
    One thing a sum cannot hand back is the sign of a zero: a term of -0.0 (tau_yz_top where jy = V = 0) added to the accumulator's
    +0.0 is +0.0, here as in k_film_partial, so the yardstick is 0.0 + term, which is the term itself for every other value."""
    r = case_runs(name)
    n = CASES[name][1]
    s, g, dA = r['series'], r['grid'], r['dA']
    val, tol = oracle_sums(r['terms'][-1], r['planes'][:5], dA)
    for k in range(1, 5):
        for j, q in enumerate(INTEGRANDS):
            got = getattr(s, q)[n - 1, k]
            assert abs(got - val[k, j]) <= tol[k, j], f"{PLANES[k]}: {q} {got!r} against {val[k, j]!r} (tolerance {tol[k, j]:.3e})"
    pairs = ((1, 2), (3, 4)) if split(g)[1] is not None else ((1, 2),)
    for a, b in pairs:
        for j, q in enumerate(INTEGRANDS):
            v = getattr(s, q)[n - 1]
            assert abs(v[a] + v[b] - v[0]) <= tol[a, j] + tol[b, j] + tol[0, j] + 4 * EPS * abs(v[0]), f"{PLANES[a]} + {PLANES[b]} against ones: {q}"
    # one-cell boxes: an odd and an even column (both halves of a pair), first and last row
    from gapflow_amd import weights
    nx, ny = g['Nx'], g['Ny']
    cells = [(1, 1), (nx, ny), (max(1, nx // 2), min(ny, 2)), (nx, max(1, ny - 1))]
    p = build(name)
    p._advance(n, honor_stop=False)
    p.set_weighted_integrals(np.stack([weights.box(g, ix, ix, iy, iy) for ix, iy in cells]))
    got = p.film_weighted()
    from gapflow_amd import _lib
    state = np.array(p.q)
    f = build(name)                             # the state assigned to a fresh problem: its derived fields are the closures OF that state
    f.q[...] = state
    lower, upper = f._derived(_lib.FIELD_WALL_LOWER), f._derived(_lib.FIELD_WALL_UPPER)
    pressure = r['terms'][-1][0] if p.prop['EOS'] == 'DH' else f._derived(_lib.FIELD_PRESSURE)[0][1:-1, 1:-1]
    h = np.array(p.topo.full[0])
    want = {'p': np.pad(pressure, 1), 'h': h, 'rho_h': state[0] * h, 'jx_h': state[1] * h, 'jy_h': state[2] * h,
            'tau_xz_bot': lower[4], 'tau_yz_bot': lower[3], 'tau_xz_top': upper[4], 'tau_yz_top': upper[3]}
    wrong = []
    for k, (ix, iy) in enumerate(cells):
        for q in INTEGRANDS:
            t = 0.0 + float(want[q][ix, iy]) * dA       # (a sum that starts at +0.0 returns +0.0 for a term of -0.0; any other term as it is)
            if bits(got[q][k]) != bits(t):
                wrong.append(f"({ix}, {iy}) {q}: {got[q][k]!r} against {t!r}")
    print(f"\n[{name}] one-cell boxes that differ from the cell's term times dA in a bit: {wrong or 'none'}")
    assert not wrong, wrong


@pytest.mark.parametrize('name', NAMES)
def test_values_match_the_oracle_sums(hiplib, name):
    """K = 8 planes (ones, four boxes, a cos and a sin mode, a smooth random plane): every integrand of every plane and recorded
    step within (1e-12 + n eps) fsum|w f| dA of the fsum of the oracle's integrands times the weights on the stepped twin's state.

    Largest |device - oracle| / tolerance over all 8 planes and all steps of a case, measured on an MI355X (the figures this
    test prints; the whole table: profiles/weighted/README.md):
        p, h, rho_h, jx_h, jy_h        <= 3.1e-4 in every case (small-1d rho_h 3.02e-4, slip-field jy_h 2.61e-4)
        wall stresses                  <= 1.9e-3 (strided-pairs tau_yz_top 1.83e-3, piezo-wide 1.12e-3), <= 8.8e-4 without
                                       piezo-viscosity (small-1d tau_xz_bot)
        0 where the integrand vanishes (jy_h, tau_yz_* on the x-only gaps)."""
    r = case_runs(name)
    s, n = r['series'], CASES[name][1]
    assert s.step.tolist() == r['twin_steps'] == list(range(1, n + 1))
    assert_bitwise(r['q'], r['twin_q'], 'final q against the stepped twin')
    worst = {q: 0.0 for q in INTEGRANDS}
    for k in range(n):
        val, tol = oracle_sums(r['terms'][k], r['planes'], r['dA'])
        for j, q in enumerate(INTEGRANDS):
            got = getattr(s, q)[k]
            assert np.all(np.isfinite(got))
            err = np.abs(got - val[:, j])
            ratio = np.where(tol[:, j] > 0, err / np.where(tol[:, j] > 0, tol[:, j], 1.0), np.where(err == 0, 0.0, np.inf))
            worst[q] = max(worst[q], float(ratio.max()))
    print(f"\n[{name}] largest |device - oracle| / tolerance over {n} steps and 8 planes: " + ', '.join(f"{q} {w:.2e}" for q, w in worst.items()))
    bad = {q: w for q, w in worst.items() if not w <= 1.0}
    assert not bad, f"{name}: outside the tolerance (error / tolerance): {bad}"


@pytest.mark.parametrize('name', NAMES)
def test_record_is_a_pure_function_of_the_state(hiplib, name):
    """The same bits from one batch, from single update() calls, at a stride of 3 picked out of a stride of 1, and from
    film_weighted() after each step."""
    r = case_runs(name)
    s, n = r['series'], CASES[name][1]
    assert_same_series(r['twin_series'], s, 'single update() calls against one batch')
    strided = armed(name, 3)
    strided._advance(n, honor_stop=False)
    pick = [k for k in range(n) if (k + 1) % 3 == 0]
    assert strided.weighted_integrals.step.tolist() == [k + 1 for k in pick]
    assert_same_series(s, strided.weighted_integrals, 'every = 1 restricted to the multiples of 3 against every = 3', pick=pick)
    for k in range(n):
        for q in INTEGRANDS:
            assert_bitwise(getattr(s, q)[k], r['now'][k][q], f"step {k + 1}: {q} recorded against film_weighted() on the twin")


@pytest.mark.parametrize('name', NAMES)
def test_recording_leaves_the_run_unchanged(hiplib, name):
    """Final q, every scalar and the whole scalar log against the same batch with nothing armed."""
    r = case_runs(name)
    assert_bitwise(r['q'], r['plain_q'], 'final q with and without weighted integrals')
    assert_same_scalars(r['scalars'], r['plain_scalars'], 'final scalars')
    assert len(r['log']) == len(r['plain_log']) == CASES[name][1]
    for i, (a, b) in enumerate(zip(r['log'], r['plain_log'])):
        assert_same_scalars(a, b, f"scalar record of step {i + 1}")


def test_cut_small_batches_at_a_stride_match_the_uncut_run(hiplib):
    """every = 7 on the small-grid kernel: pieces of 7, 7, ... and a remainder against one launch."""
    r = case_runs('small-1d')
    p = armed('small-1d', 7)
    log = p._advance(50, honor_stop=False)
    assert p.weighted_integrals.step.tolist() == [7, 14, 21, 28, 35, 42, 49]
    assert_bitwise(p.q, r['plain_q'], 'final q')
    assert_same_scalars(scalars_of(p), r['plain_scalars'], 'final scalars')
    for i, (e, b) in enumerate(zip(log, r['plain_log'])):
        assert_same_scalars(tuple(getattr(e, k) for k in SCALARS), b, f"scalar record of step {i + 1}")
    assert_same_series(r['series'], p.weighted_integrals, 'every = 7 against every = 1', pick=[6, 13, 20, 27, 34, 41, 48])


def test_series_armed_together_at_different_strides_equal_each_alone(hiplib):
    """small-1d with film integrals (2), weighted integrals (3), extrema (5) and probes armed at once -- the batch is cut at the
    union of the multiples of 2 and 3 -- against each series recorded with only that series armed; the run itself unchanged."""
    r = case_runs('small-1d')
    n = CASES['small-1d'][1]
    both = armed('small-1d', 3)
    both.set_integrals(2)
    both.set_extrema(5)
    both.set_probes(tp.CELLS_1D, pressure=True)
    log = both._advance(n, honor_stop=False)
    assert_bitwise(both.q, r['plain_q'], 'final q')
    for i, (e, b) in enumerate(zip(log, r['plain_log'])):
        assert_same_scalars(tuple(getattr(e, k) for k in SCALARS), b, f"scalar record of step {i + 1}")
    assert_same_series(r['series'], both.weighted_integrals, 'weighted integrals at 3', pick=[k for k in range(n) if (k + 1) % 3 == 0])
    integ = build('small-1d')
    integ.set_integrals(2)
    integ._advance(n, honor_stop=False)
    assert both.integrals.step.tolist() == integ.integrals.step.tolist() == list(range(2, n + 1, 2))
    for q in ('time', 'load', 'load_x', 'p_hx', 'tau_xz_bot', 'tau_xz_top', 'flow_x', 'flow_y'):
        assert_bitwise(getattr(both.integrals, q), getattr(integ.integrals, q), f"film integrals at 2: {q}")
    extr = build('small-1d')
    extr.set_extrema(5)
    extr._advance(n, honor_stop=False)
    assert both.extrema.step.tolist() == extr.extrema.step.tolist() == list(range(5, n + 1, 5))
    for q in ('time', 'p_max', 'p_min', 'rho_max', 'rho_min', 'h_min', 'u_max', 'v_max'):
        assert_bitwise(getattr(both.extrema, q), getattr(extr.extrema, q), f"extrema at 5: {q}")
    assert both.extrema.cells.tolist() == extr.extrema.cells.tolist()
    alone = tp.case_runs('small-1d')['series']
    assert both.probes.step.tolist() == alone.step.tolist()
    for q in ('time', 'rho', 'jx', 'jy', 'p'):
        assert_bitwise(getattr(both.probes, q), getattr(alone, q), f"probes: {q}")


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_max_it_under_honor_stop_ends_the_series(hiplib, name):
    text = CASES[name][0]
    for every, want in ((1, list(range(1, 8))), (2, [2, 4, 6]), (7, [7]), (8, [])):
        p = tp.build(text.replace('max_it: 100000', 'max_it: 7'))
        p.set_weighted_integrals(planes_of(p)[[0, 5]], every)
        p._advance(20, honor_stop=True)
        s = p.weighted_integrals
        assert p.step == 7 and s.step.tolist() == want and s.p.shape == (len(want), 2) and s.names == ('w0', 'w1')
        if every == 7:
            now = p.film_weighted()
            for q in INTEGRANDS:
                assert_bitwise(getattr(s, q)[0], now[q], f"last record against the state the run ended on: {q}")


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_rolled_back_step_leaves_no_record(hiplib, name):
    """tests/test_gpu_parity.py: test_invalid_state_rolls_back's way to an invalid state (an absurd time step): the scalar log
    keeps its entry for the invalid step, the series ends one entry before it, and film_weighted() refuses the flagged state."""
    from gapflow_amd import _lib
    p = armed(name)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_weighted_read(p._h, None, 0, None, C.byref(have)))
    assert have.value == 0
    np.testing.assert_array_equal(p.q, good)
    assert p.weighted_integrals.step.tolist() == [1, 2, 3]
    ref = case_runs(name)['series']
    for n, x in series_arrays(p.weighted_integrals):
        assert_bitwise(x, getattr(ref, n)[:3], f"records before the rollback: {n}")
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.film_weighted()


def test_refusals(hiplib):
    from gapflow_amd import Ensemble, Problem, _lib
    p = tp.build(SLIDER_2D)
    nx, ny = p.grid['Nx'], p.grid['Ny']
    ones = np.ones((nx, ny))
    ghosted = np.ones((9, nx + 2, ny + 2))
    # K and shape
    with pytest.raises(ValueError, match='0 weight planes, 1 to 8 required'):
        p.set_weighted_integrals(np.ones((0, nx, ny)))
    with pytest.raises(ValueError, match='9 weight planes, 1 to 8 required'):
        p.set_weighted_integrals(np.ones((9, nx, ny)))
    with pytest.raises(ValueError, match=rf'\(K, {nx}, {ny}\)'):
        p.set_weighted_integrals(np.ones((nx + 2, ny + 2)))
    with pytest.raises(ValueError, match='stride'):
        p.set_weighted_integrals(ones, 0)
    assert p.weighted_integrals is None
    with pytest.raises(RuntimeError, match='no weights are set'):
        p.film_weighted()
    for K in (0, 9):
        assert p._lib.gpf_weighted_set(p._h, 1, K, _lib.as_dp(ghosted)) == -1
        assert f'1 to 8 weight planes required, got {K}'.encode() in p._lib.gpf_last_error()
    assert p._lib.gpf_weighted_set(p._h, 0, 1, _lib.as_dp(ghosted)) == -1 and b'every >= 1' in p._lib.gpf_last_error()
    assert p._lib.gpf_weighted_read(p._h, None, 0, None, None) == -5
    out = np.empty(72)
    assert p._lib.gpf_weighted_now(p._h, _lib.as_dp(out), 72) == -5 and b'no weighted integrals are armed' in p._lib.gpf_last_error()
    # a weight that is not finite: plane and cell named, by the host check of the package and by the library's own
    w = np.ones((3, nx, ny))
    w[2, 36, 4] = np.nan
    with pytest.raises(ValueError, match=r'weight plane 2 is not finite at cell \(37, 5\)'):
        p.set_weighted_integrals(w)
    ghosted[1, 37, 5] = np.inf
    assert p._lib.gpf_weighted_set(p._h, 1, 3, _lib.as_dp(ghosted)) == -1
    assert b'weight plane 1 is not finite at cell (37, 5)' in p._lib.gpf_last_error()
    ghosted[1, 37, 5] = 1.0
    ghosted[0, 0, 0] = np.nan                   # a ghost entry is ignored, whatever it holds
    _lib.check(p._lib.gpf_weighted_set(p._h, 1, 1, _lib.as_dp(ghosted)))
    small = np.empty(8)
    assert p._lib.gpf_weighted_now(p._h, _lib.as_dp(small), 8) == -1 and b'room for 9 doubles' in p._lib.gpf_last_error()
    _lib.check(p._lib.gpf_weighted_now(p._h, _lib.as_dp(out), 72))
    assert np.all(np.isfinite(out[:9]))
    _lib.check(p._lib.gpf_weighted_clear(p._h))
    # an open stage-wise step
    _lib.check(p._lib.gpf_open_step(p._h))
    assert p._lib.gpf_weighted_set(p._h, 1, 1, _lib.as_dp(ghosted)) == -5 and b'stage-wise step is open' in p._lib.gpf_last_error()
    for i in range(2):
        _lib.check(p._lib.gpf_stage_closures(p._h))
        _lib.check(p._lib.gpf_stage_advance(p._h, i))
    sc = _lib.GpfScalars()
    _lib.check(p._lib.gpf_close_step(p._h, C.byref(sc)))
    p.set_weighted_integrals(ones, 2)           # closed: armed; gpf_close_step itself records nothing
    assert p.weighted_integrals.step.shape == (0,) and p.weighted_integrals.p.shape == (0, 1)
    # shear thinning
    t = tp.build(THINNING)
    tw = np.ones((t.grid['Nx'], t.grid['Ny']))
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.set_weighted_integrals(tw)
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.film_weighted()
    tg = np.ones((1, t.grid['Nx'] + 2, t.grid['Ny'] + 2))
    assert t._lib.gpf_weighted_set(t._h, 1, 1, _lib.as_dp(tg)) == -1 and b'shear thinning' in t._lib.gpf_last_error()
    # an elastic gap
    e = tp.build(ELASTIC)
    with pytest.raises(NotImplementedError, match='elastic gap'):
        e.set_weighted_integrals(np.ones((e.grid['Nx'], e.grid['Ny'])))
    eg = np.ones((1, e.grid['Nx'] + 2, e.grid['Ny'] + 2))
    assert e._lib.gpf_weighted_set(e._h, 1, 1, _lib.as_dp(eg)) == -1 and b'elastic handle' in e._lib.gpf_last_error()
    # surrogate closures
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = quiet(Problem.from_string, SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            g.set_weighted_integrals(np.ones((g.grid['Nx'], g.grid['Ny'])))
        quiet(g._pre_run)
        gg = np.ones((1, g.grid['Nx'] + 2, g.grid['Ny'] + 2))
        assert g._lib.gpf_weighted_set(g._h, 1, 1, _lib.as_dp(gg)) == -1 and b'surrogate' in g._lib.gpf_last_error()
    # an armed member of an ensemble: member and reason named, by the package and by the library
    members = [tp.build(JOURNAL_1D), tp.build(JOURNAL_1D.replace('eps: 0.7', 'eps: 0.5'))]
    members[1].set_weighted_integrals(np.ones((100, 1)))
    with pytest.raises(NotImplementedError, match='member 1: weighted integrals are armed'):
        Ensemble(members)
    handles = (C.c_void_p * 2)(*[m._h.value for m in members])
    ens = C.c_void_p()
    assert members[0]._lib.gpf_ensemble_create(handles, 2, C.byref(ens)) == -1
    assert b'member 1: weighted integrals are armed on it' in members[0]._lib.gpf_last_error()
    members[1].clear_weighted_integrals()
    made = Ensemble(members)
    members[0].set_weighted_integrals(np.ones((100, 1)))
    with pytest.raises(NotImplementedError, match='member 0: .*weighted integrals are armed'):
        made.step(3)


def run_yaml(out, silent, max_it=12):
    options = (f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, weighted_integrals: 3, "
               f"weights: [{{box: [1, 50, 1, 1], name: pad0}}, {{box: [51, 100, 1, 1], name: pad1}}, {{mode: [1, 0, sin]}}, {{file: w.npy, name: ones}}]}}")
    return JOURNAL_1D.replace("options: {silent: True}", options).replace('max_it: 100000', f'max_it: {max_it}')


def test_run_writes_weighted_npz_and_a_restored_problem_rearms(hiplib, tmp_path):
    from gapflow_amd import Problem
    np.save(tmp_path / 'w.npy', np.ones((100, 1)))
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False), base_dir=str(tmp_path))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'weighted.npz'))
    assert sorted(f.files) == sorted(('step', 'time', 'names') + INTEGRANDS)
    assert f['names'].tolist() == ['pad0', 'pad1', 'w2', 'ones'] and f['step'].tolist() == [3, 6, 9, 12] and f['p'].shape == (4, 4)
    ref = case_runs('small-1d')['series']                   # the same problem, every = 1: plane 0 is ones
    for q in INTEGRANDS:
        assert_bitwise(f[q][:, 3], getattr(ref, q)[[2, 5, 8, 11], 0], f"run() at stride 3 against the batch at stride 1, the ones plane: {q}")
    assert_bitwise(f['time'], ref.time[[2, 5, 8, 11]], 'time')
    assert np.all(np.abs(f['p'][:, 0] + f['p'][:, 1] - f['p'][:, 3]) <= 4 * EPS * np.abs(f['p'][:, 3]))       # two pads carry the film's load
    # checkpoints do not carry the series: the restored problem re-arms from its options and records from the restart step
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000), base_dir=str(tmp_path))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(7, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.weighted_integrals.step.shape == (0,) and b.weighted_integrals.names == ('pad0', 'pad1', 'w2', 'ones')
    b._advance(7, honor_stop=False)
    assert a.weighted_integrals.step.tolist() == [3, 6, 9, 12] and b.weighted_integrals.step.tolist() == [6, 9, 12]
    for n, x in series_arrays(b.weighted_integrals):
        assert_bitwise(x, dict(series_arrays(a.weighted_integrals))[n][1:], f"restored against continued: {n}")
    b.clear_weighted_integrals()
    assert b.weighted_integrals is None
