"""Region series (gpf_regions_*, Problem.set_regions / regions / film_regions, options.regions + options.region_list): the weighted
film integrals' nine sums over zones the state defines -- a field inside [lo, hi), inside a box --, the zone's exact cell count and
its bounding box, reduced on the device while gpf_step advances whole batches.

Inputs: the cases of tests/test_gpu_integrals.py (Ny = 1, 300, 601 -- odd, more than one column pair per thread --, a slip-length
field, the row-coefficient and the planes topographies) and one grid of 300 x 5 (Nx > 256: k_region_fold's threads take a second
row).  Yardsticks:
  * Problem.film_weighted() of a twin armed with the 0 / 1 planes NumPy builds from the downloaded state with the same predicate,
    bit for bit, all nine integrands: the region kernels add through the weighted kernels' own functions in their own order with
    a weight of exactly 1.0 or 0.0;
  * NumPy's count and bounding box of those planes, exactly;
  * math.fsum of the oracle's integrands on the NumPy mask, tolerance (1e-12 + n eps) fsum|w f| dA --
    tests/test_gpu_weighted.py: test_values_match_the_oracle_sums' rule, unchanged;
  * everything else bit for bit: a record is a pure function of the state and the region list, and recording only reads.
Reference: none (post-processing there)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import test_gpu_probes as tp
from test_gpu_integrals import CASES, build
from test_gpu_probes import (JOURNAL_1D, SCALARS, SLIDER_2D, SURROGATE, THINNING, assert_bitwise, assert_same_scalars, bits, quiet,
                             scalars_of)
from test_gpu_weighted import ELASTIC, INTEGRANDS, oracle_sums, oracle_terms

pytestmark = pytest.mark.gpu

INF = float('inf')
# 300 x 5: off the small-grid kernel (302 x 7 cells x 16 doubles > 150 KB), Nx > 256: k_region_fold's second trip over the rows
WIDE_ROWS = tp.TWO_D.format(bc=tp.DN + ", xE_D: 877.7007, xW_D: 876.", geo="{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.05}") \
    .replace('Nx: 128, Ny: 130', 'Nx: 300, Ny: 5').replace('Lx: 0.02, Ly: 0.03', 'Lx: 0.03, Ly: 0.0005')
STEPS = dict({name: c[1] for name, c in CASES.items()}, **{'wide-rows': 6})
NAMES = list(STEPS)
NAMED = ('rho_from', 'rho_below', 'h_band_box', 'jx_from', 'jy_below', 'p_from', 'all', 'none')
INTS = ('cells', 'bbox')


def make(name):
    return tp.build(WIDE_ROWS) if name == 'wide-rows' else build(name)


def middle(f, at):
    """A value some interior cell holds itself: the one `at` of the way through the sorted interior values."""
    v = np.sort(np.asarray(f)[1:-1, 1:-1].ravel())
    return float(v[min(v.size - 1, int(at * v.size))])


def regions_of(q, h, pcell):
    """The K = 8 regions of NAMED for a downloaded state: bounds that ARE cells' own values -- a lower bound includes its cell, an
    upper bound excludes it --, one band with a box that cuts a column pair in the middle, the whole interior, and nothing."""
    nx, ny = q.shape[1] - 2, q.shape[2] - 2
    hlo, hhi = middle(h, 0.25), middle(h, 0.75)
    box = [max(1, nx // 4), max(1, nx - nx // 3), 2 if ny > 2 else 1, max(1, ny - 1)]
    return [{'field': 'rho', 'above': middle(q[0], 0.5), 'name': NAMED[0]},
            {'field': 'rho', 'below': middle(q[0], 0.5), 'name': NAMED[1]},
            {'field': 'h', 'above': hlo, 'below': hhi if hhi > hlo else INF, 'box': box, 'name': NAMED[2]},
            {'field': 'jx', 'above': middle(q[1], 0.3), 'name': NAMED[3]},
            {'field': 'jy', 'below': middle(q[2], 0.6), 'name': NAMED[4]},
            {'field': 'p', 'above': middle(pcell, 0.7), 'name': NAMED[5]},
            {'field': 'h', 'name': NAMED[6]},
            {'field': 'rho', 'above': 1.e30, 'name': NAMED[7]}]


def masks_of(regions, q, h, pcell):
    """(K, Nx, Ny) bool: the predicate restated in NumPy on the interior cells."""
    fields = {'rho': q[0], 'jx': q[1], 'jy': q[2], 'h': h, 'p': pcell}
    nx, ny = q.shape[1] - 2, q.shape[2] - 2
    ix, iy = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), indexing='ij')
    out = []
    for r in regions:
        f = np.asarray(fields[r['field']])[1:-1, 1:-1]
        b = r.get('box') or (1, nx, 1, ny)
        out.append((r.get('above', -INF) <= f) & (f < r.get('below', INF)) & (b[0] <= ix) & (ix <= b[1]) & (b[2] <= iy) & (iy <= b[3]))
    return np.stack(out)


def bbox_of(mask):
    if not mask.any():
        return [-1, -1, -1, -1]
    ix, iy = np.nonzero(mask)
    return [int(ix.min()) + 1, int(ix.max()) + 1, int(iy.min()) + 1, int(iy.max()) + 1]


def state_of(p):
    return np.array(p.q), np.array(p.topo.full[0])


@functools.lru_cache(maxsize=None)
def case_state(name):
    """A problem stepped the case's steps, the last one with a one-record statistics window of p (its p_min is the per-cell p of
    the committed state) and the extrema armed; the state downloaded; the regions and their NumPy masks; film_regions() of it; a
    twin stepped alike with the masks armed as weight planes: film_weighted(); film_integrals() and the oracle's integrands."""
    n = STEPS[name]
    p, twin = make(name), make(name)
    p._advance(n - 1, honor_stop=False)
    p.set_statistics(1, ('p',))
    p._advance(1, honor_stop=False)
    st = p.statistics
    assert st['count'] == 1 and st['last_step'] == n
    pcell = np.array(st['p_min'])
    p.clear_statistics()
    q, h = state_of(p)
    regions = regions_of(q, h, pcell)
    masks = masks_of(regions, q, h, pcell)
    p.set_regions(regions)
    now = p.film_regions()
    extrema = p.field_extrema()
    p.set_regions([{'field': 'p', 'above': float(extrema['p_max'])}])
    peak = p.film_regions()
    twin._advance(n, honor_stop=False)
    assert_bitwise(twin.q, q, 'the twin\'s state')
    twin.set_weighted_integrals(masks.astype(np.float64))
    return dict(q=q, h=h, pcell=pcell, regions=regions, masks=masks, now=now, weighted=twin.film_weighted(), integrals=twin.film_integrals(),
                extrema=extrema, peak=peak, terms=oracle_terms(twin), grid=dict(p.grid), dA=p.grid['dx'] * p.grid['dy'])


@pytest.mark.parametrize('name', NAMES)
def test_sums_equal_the_weighted_integrals_of_the_mask_bit_for_bit(hiplib, name):
    """rho, h, jx, jy and p regions -- lower bounds that equal a cell's own value (included), upper bounds that do (excluded), one
    box --: all nine integrands of film_regions() against film_weighted() of the twin armed with the NumPy masks, every bit."""
    r = case_state(name)
    m = r['masks']
    print(f"\n[{name}] cells per region: {dict(zip(NAMED, m.reshape(len(m), -1).sum(axis=1).tolist()))}")
    q, regions = r['q'], r['regions']
    assert (q[0][1:-1, 1:-1] == regions[0]['above']).any() and m[0][q[0][1:-1, 1:-1] == regions[0]['above']].all()        # lo: its cell is in
    assert (q[0][1:-1, 1:-1] == regions[1]['below']).any() and not m[1][q[0][1:-1, 1:-1] == regions[1]['below']].any()   # hi: its cell is out
    assert not (m[0] & m[1]).any() and (m[0] | m[1]).all()
    for k in INTEGRANDS:
        assert r['now'][k].shape == (8,)
        assert_bitwise(r['now'][k], r['weighted'][k], f"{k}: regions against the weighted integrals of their masks")


@pytest.mark.parametrize('name', ['strided-pairs', 'slip-field', 'small-1d', 'wide-rows'])
def test_narrow_loads_give_the_same_bits(hiplib, name, monkeypatch):
    """GPF_FILM_NARROW (read by gpf_regions_set and gpf_weighted_set): the 8-byte loads -- an odd Ny walked in strides, a slip-length
    field, Ny = 1 -- against the wide loads' record and against the weighted integrals read with 8-byte loads too."""
    r = case_state(name)                            # wide loads: computed before the variable is set, or by an earlier test
    monkeypatch.setenv('GPF_FILM_NARROW', '1')
    p = make(name)
    p._advance(STEPS[name], honor_stop=False)
    p.set_regions(r['regions'])
    p.set_weighted_integrals(r['masks'].astype(np.float64))
    now, w = p.film_regions(), p.film_weighted()
    for k in INTEGRANDS:
        assert_bitwise(now[k], r['now'][k], f"{k}: 8-byte loads against 16-byte loads")
        assert_bitwise(now[k], w[k], f"{k}: regions against weighted integrals, both with 8-byte loads")
    for k in INTS:
        assert now[k].tolist() == r['now'][k].tolist(), k


@pytest.mark.parametrize('name', NAMES)
def test_count_and_bounding_box(hiplib, name):
    """cells and bbox against NumPy's of the masks; the region nothing satisfies: 0 cells, bbox -1, nine sums of +0.0 with the sign
    bit clear; (-inf, +inf) over the interior: Nx Ny cells and `load` / tau_* of the film integrals in every bit; p >= p_max of
    the extrema record of the same state: at least one cell, and its bbox holds the extrema's cell."""
    r = case_state(name)
    g, now, m = r['grid'], r['now'], r['masks']
    assert now['cells'].dtype == np.int64 and now['bbox'].shape == (8, 4)
    assert now['cells'].tolist() == [int(x.sum()) for x in m]
    assert now['bbox'].tolist() == [bbox_of(x) for x in m]
    assert_bitwise(now['area'], now['cells'] * (g['dx'] * g['dy']), 'area')
    none, whole = NAMED.index('none'), NAMED.index('all')
    assert now['cells'][none] == 0 and now['bbox'][none].tolist() == [-1, -1, -1, -1]
    for k in INTEGRANDS:
        assert bits(now[k][none]) == 0, f"{k} of the empty region: {now[k][none]!r} (bits {int(bits(now[k][none])):#x})"
    assert now['cells'][whole] == g['Nx'] * g['Ny'] and now['bbox'][whole].tolist() == [1, g['Nx'], 1, g['Ny']]
    for mine, theirs in (('p', 'load'), ('tau_xz_bot', 'tau_xz_bot'), ('tau_yz_bot', 'tau_yz_bot'), ('tau_xz_top', 'tau_xz_top'),
                         ('tau_yz_top', 'tau_yz_top')):
        assert_bitwise(now[mine][whole], r['integrals'][theirs], f"the whole interior: {mine} against the integrals' {theirs}")
    peak, (ix, iy) = r['peak'], r['extrema']['p_max_cell']
    b = peak['bbox'][0]
    assert peak['cells'][0] >= 1 and b[0] <= ix <= b[1] and b[2] <= iy <= b[3], (peak['cells'], b, (ix, iy))
    assert peak['cells'][0] == int((r['pcell'][1:-1, 1:-1] >= r['extrema']['p_max']).sum())


@pytest.mark.parametrize('name', NAMES)
def test_values_match_the_oracle_sums_on_the_mask(hiplib, name):
    """Every integrand of every region within (1e-12 + n eps) fsum|w f| dA of the fsum of the oracle's integrands on the NumPy
    mask: tests/test_gpu_weighted.py: test_values_match_the_oracle_sums' rule and tolerance."""
    r = case_state(name)
    val, tol = oracle_sums(r['terms'], r['masks'].astype(np.float64), r['dA'])
    worst = {}
    for j, k in enumerate(INTEGRANDS):
        got = r['now'][k]
        assert np.all(np.isfinite(got))
        err = np.abs(got - val[:, j])
        ratio = np.where(tol[:, j] > 0, err / np.where(tol[:, j] > 0, tol[:, j], 1.0), np.where(err == 0, 0.0, np.inf))
        worst[k] = float(ratio.max())
    print(f"\n[{name}] largest |device - oracle| / tolerance over 8 regions: " + ', '.join(f"{k} {w:.2e}" for k, w in worst.items()))
    bad = {k: w for k, w in worst.items() if not w <= 1.0}
    assert not bad, f"{name}: outside the tolerance (error / tolerance): {bad}"


# ---- series ------------------------------------------------------------------------------------------------------------

RHO_UP = 877.701        # small-1d: see test_the_region_follows_the_state
SERIES_REGIONS = [{'field': 'rho', 'above': RHO_UP, 'name': 'compressed'}, {'field': 'p', 'below': 101325.0, 'box': [10, 90, 1, 1], 'name': 'below_p0'},
                  {'field': 'jx', 'above': 0.0, 'name': 'forward'}]


def armed(name, every=1, regions=SERIES_REGIONS):
    p = make(name)
    p.set_regions(regions, every)
    return p


def series_arrays(s):
    return [(n, getattr(s, n)) for n in ('time',) + INTEGRANDS + ('area',)]


def assert_same_series(a, b, what, pick=None):
    """Bitwise; `pick`: indices of a's records to hold against all of b's."""
    sel = (lambda v: v[pick]) if pick is not None else (lambda v: v)
    assert sel(a.step).tolist() == b.step.tolist(), what
    assert a.names == b.names
    for (n, x), (_, y) in zip(series_arrays(a), series_arrays(b)):
        assert_bitwise(sel(x), y, f"{what}: {n}")
    for n in INTS:
        assert sel(getattr(a, n)).tolist() == getattr(b, n).tolist(), f"{what}: {n}"


@functools.lru_cache(maxsize=None)
def series_runs(name):
    """One recorded batch (every = 1); a twin advanced by single update() calls (its series, film_regions() and the state after
    every step); the same batch with nothing armed.  Computed once per case and only read by the tests."""
    n = STEPS[name]
    rec, twin, plain = armed(name), armed(name), make(name)
    log = rec._advance(n, honor_stop=False)
    plain_log = plain._advance(n, honor_stop=False)
    now, states = [], []
    for _ in range(n):
        twin.update()
        now.append(twin.film_regions())
        states.append(np.array(twin.q))
    return dict(series=rec.regions, q=rec.q.copy(), scalars=scalars_of(rec), log=[tuple(getattr(e, k) for k in SCALARS) for e in log],
                plain_q=plain.q.copy(), plain_scalars=scalars_of(plain), plain_log=[tuple(getattr(e, k) for k in SCALARS) for e in plain_log],
                twin_series=twin.regions, now=now, states=states)


def test_the_region_follows_the_state(hiplib):
    """small-1d (the journal bearing starting from rest at rho0 = 877.7007, 50 steps), region rho >= 877.701: picked on the CPU
    oracle (oracle/problem.py: OracleProblem stepped 50 times, the predicate restated in NumPy on its states), where the zone is
    empty for the steps 1 .. 5 and then grows: 5 cells after step 6, 14, 18, 22, 25 after the steps 7 .. 10, 33 after step 15,
    38 after step 21, 44 after step 50.  Here the device's count must equal NumPy's on the state read after every single
    update(), and take at least two values over the series -- a test on a mask that never changes shows nothing."""
    r = series_runs('small-1d')
    s = r['series']
    want = [int((q[0][1:-1, 1:-1] >= RHO_UP).sum()) for q in r['states']]
    print(f"\ncells of rho >= {RHO_UP} after the steps 1 .. {len(want)}: {want}")
    assert s.names[0] == 'compressed' and s.cells[:, 0].tolist() == want
    assert len(set(want)) >= 2 and want[0] == 0 and want[-1] > 0
    assert s.bbox[0, 0].tolist() == [-1, -1, -1, -1] and s.bbox[-1, 0, 2:].tolist() == [1, 1]
    assert all(bits(getattr(s, k)[0, 0]) == 0 for k in INTEGRANDS)


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef', 'wide-rows'])
def test_record_is_a_pure_function_of_the_state(hiplib, name):
    """The same bits from one batch, from single update() calls, at a stride of 3 picked out of a stride of 1, and from
    film_regions() after each step."""
    r = series_runs(name)
    s, n = r['series'], STEPS[name]
    assert s.step.tolist() == list(range(1, n + 1)) and s.p.shape == (n, 3) and s.cells.shape == (n, 3) and s.bbox.shape == (n, 3, 4)
    assert_same_series(r['twin_series'], s, 'single update() calls against one batch')
    strided = armed(name, 3)
    strided._advance(n, honor_stop=False)
    pick = [k for k in range(n) if (k + 1) % 3 == 0]
    assert strided.regions.step.tolist() == [k + 1 for k in pick]
    assert_same_series(s, strided.regions, 'every = 1 restricted to the multiples of 3 against every = 3', pick=pick)
    for k in range(n):
        for q in INTEGRANDS + ('area',):
            assert_bitwise(getattr(s, q)[k], r['now'][k][q], f"step {k + 1}: {q} recorded against film_regions() on the twin")
        for q in INTS:
            assert getattr(s, q)[k].tolist() == r['now'][k][q].tolist()


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef', 'wide-rows'])
def test_recording_leaves_the_run_unchanged(hiplib, name):
    """Final q, every scalar and the whole scalar log against the same batch with nothing armed."""
    r = series_runs(name)
    assert_bitwise(r['q'], r['plain_q'], 'final q with and without regions')
    assert_same_scalars(r['scalars'], r['plain_scalars'], 'final scalars')
    assert len(r['log']) == len(r['plain_log']) == STEPS[name]
    for i, (a, b) in enumerate(zip(r['log'], r['plain_log'])):
        assert_same_scalars(a, b, f"scalar record of step {i + 1}")


CHILD = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import test_gpu_probes as tp
import test_gpu_regions as tr
states, out = np.load(sys.argv[1]), sys.argv[2]
p = tr.armed('small-1d', 7)
log = p._advance(14, honor_stop=False)          # k_step2, one launch per step: the series of this form, against its own film_regions()
own = p.regions
assert own.step.tolist() == [7, 14]
now = p.film_regions()
for k in tr.INTEGRANDS:
    tp.assert_bitwise(getattr(own, k)[1], now[k], k)
assert own.cells[1].tolist() == now['cells'].tolist() and own.bbox[1].tolist() == now['bbox'].tolist()
res = {}
for key in states.files:                         # the other form's states: the record is a function of the state alone
    p.q[...] = states[key]
    rec = p.film_regions()
    for k in tr.INTEGRANDS + tr.INTS:
        res[key + '_' + k] = rec[k]
np.savez(out, **res)
'''


def test_cut_small_batches_match_the_uncut_run_and_the_launch_per_step_form(hiplib, tmp_path):
    """every = 7 on the one-workgroup kernel: pieces of 7, 7, ... and a remainder against one launch -- the uncut run's q, scalars
    and log in every bit, and the records of every = 1 at the multiples of 7.  The same run with GPF_SMALL_GRID=0 (a child process:
    the switch is read once per process) goes through k_step2 with one recording launch behind each step; the two forms sum the
    step's scalars in different orders (tests/test_gpu_extras.py holds their states to 1e-10), so what must be equal there in
    every bit is the record of the SAME state: the child is handed the states this form recorded at and returns film_regions()
    of each, and checks its own batch against its own film_regions()."""
    r = series_runs('small-1d')
    p = armed('small-1d', 7)
    log = p._advance(50, honor_stop=False)
    assert p.regions.step.tolist() == [7, 14, 21, 28, 35, 42, 49]
    assert_bitwise(p.q, r['plain_q'], 'final q')
    assert_same_scalars(scalars_of(p), r['plain_scalars'], 'final scalars')
    for i, (e, b) in enumerate(zip(log, r['plain_log'])):
        assert_same_scalars(tuple(getattr(e, k) for k in SCALARS), b, f"scalar record of step {i + 1}")
    pick = [6, 13, 20, 27, 34, 41, 48]
    assert_same_series(r['series'], p.regions, 'every = 7 against every = 1', pick=pick)
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez(tmp_path / 'states.npz', **{f's{k + 1}': r['states'][k] for k in pick})
    res = subprocess.run([sys.executable, '-c', CHILD % dict(root=os.path.dirname(here), tests=here), str(tmp_path / 'states.npz'), str(tmp_path / 'child.npz')],
                         env=dict(os.environ, GPF_SMALL_GRID='0'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(tmp_path / 'child.npz')
    for i, k in enumerate(pick):
        for q in INTEGRANDS:
            assert_bitwise(got[f's{k + 1}_{q}'], getattr(p.regions, q)[i], f"step {k + 1}: {q} through the launch-per-step form")
        for q in INTS:
            assert got[f's{k + 1}_{q}'].tolist() == getattr(p.regions, q)[i].tolist()


def test_series_armed_together_at_different_strides_equal_each_alone(hiplib):
    """small-1d with film integrals (2), weighted integrals (3) and regions (5) armed at once -- the batch is cut at the union of
    their steps -- against each series recorded with only that series armed; the run itself unchanged."""
    r = series_runs('small-1d')
    n = STEPS['small-1d']
    w = np.stack([np.ones((100, 1)), (np.arange(100) < 40).astype(np.float64)[:, None]])
    both = armed('small-1d', 5)
    both.set_integrals(2)
    both.set_weighted_integrals(w, 3)
    log = both._advance(n, honor_stop=False)
    assert_bitwise(both.q, r['plain_q'], 'final q')
    for i, (e, b) in enumerate(zip(log, r['plain_log'])):
        assert_same_scalars(tuple(getattr(e, k) for k in SCALARS), b, f"scalar record of step {i + 1}")
    assert_same_series(r['series'], both.regions, 'regions at 5', pick=[k for k in range(n) if (k + 1) % 5 == 0])
    integ = make('small-1d')
    integ.set_integrals(2)
    integ._advance(n, honor_stop=False)
    assert both.integrals.step.tolist() == integ.integrals.step.tolist() == list(range(2, n + 1, 2))
    for q in ('time', 'load', 'load_x', 'p_hx', 'tau_xz_bot', 'tau_xz_top', 'flow_x', 'flow_y'):
        assert_bitwise(getattr(both.integrals, q), getattr(integ.integrals, q), f"film integrals at 2: {q}")
    wt = make('small-1d')
    wt.set_weighted_integrals(w, 3)
    wt._advance(n, honor_stop=False)
    assert both.weighted_integrals.step.tolist() == wt.weighted_integrals.step.tolist() == list(range(3, n + 1, 3))
    for q in ('time',) + INTEGRANDS:
        assert_bitwise(getattr(both.weighted_integrals, q), getattr(wt.weighted_integrals, q), f"weighted integrals at 3: {q}")


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_max_it_under_honor_stop_ends_the_series(hiplib, name):
    text = CASES[name][0]
    for every, want in ((1, list(range(1, 8))), (2, [2, 4, 6]), (7, [7]), (8, [])):
        p = tp.build(text.replace('max_it: 100000', 'max_it: 7'))
        p.set_regions(SERIES_REGIONS[:2], every)
        p._advance(20, honor_stop=True)
        s = p.regions
        assert p.step == 7 and s.step.tolist() == want and s.p.shape == (len(want), 2) and s.bbox.shape == (len(want), 2, 4)
        assert s.names == ('compressed', 'below_p0')
        if every == 7:
            now = p.film_regions()
            for q in INTEGRANDS:
                assert_bitwise(getattr(s, q)[0], now[q], f"last record against the state the run ended on: {q}")
            assert s.cells[0].tolist() == now['cells'].tolist()


@pytest.mark.parametrize('name', ['small-1d', 'slider-rowcoef'])
def test_rolled_back_step_leaves_no_record(hiplib, name):
    """tests/test_gpu_weighted.py: test_rolled_back_step_leaves_no_record's way to an invalid state (an absurd time step): the
    scalar log keeps its entry for the invalid step, the series ends one entry before it, and film_regions() refuses the state."""
    from gapflow_amd import _lib
    p = armed(name)
    p._advance(3, honor_stop=False)
    good = p.q.copy()
    p._lib.gpf_set_dt(p._h, 1.0)
    p.dt = 1.0
    quiet(p._advance, 5, honor_stop=False)
    assert p._stop and p.step == 3
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_regions_read(p._h, None, None, 0, None, C.byref(have)))
    assert have.value == 0
    np.testing.assert_array_equal(p.q, good)
    assert p.regions.step.tolist() == [1, 2, 3]
    ref = series_runs(name)['series']
    for n, x in series_arrays(p.regions):
        assert_bitwise(x, getattr(ref, n)[:3], f"records before the rollback: {n}")
    assert p.regions.cells.tolist() == ref.cells[:3].tolist() and p.regions.bbox.tolist() == ref.bbox[:3].tolist()
    with pytest.raises(_lib.GapflowHipError, match='flagged invalid'):
        p.film_regions()


def region_array(*regions):
    from gapflow_amd import _lib
    arr = (_lib.GpfRegion * len(regions))()
    for a, (field, lo, hi, box) in zip(arr, regions):
        a.field, a.lo, a.hi = field, lo, hi
        a.box[:] = box
    return arr


def test_refusals(hiplib):
    from gapflow_amd import Ensemble, Problem, _lib
    p = tp.build(SLIDER_2D)
    nx, ny = p.grid['Nx'], p.grid['Ny']
    whole = (0, 0, 0, 0)
    ok = region_array((1, -INF, INF, whole))
    err = p._lib.gpf_last_error
    # the package's own checks
    with pytest.raises(ValueError, match='a list of 1 to 8 regions'):
        p.set_regions([])
    with pytest.raises(ValueError, match='a list of 1 to 8 regions'):
        p.set_regions([{'field': 'rho'}] * 9)
    with pytest.raises(ValueError, match='stride'):
        p.set_regions([{'field': 'rho'}], 0)
    with pytest.raises(ValueError, match=r'entry 0: box'):
        p.set_regions([{'field': 'rho', 'box': [1, nx + 1, 1, ny]}])
    assert p.regions is None
    with pytest.raises(RuntimeError, match='no regions are set'):
        p.film_regions()
    # the library's
    for K in (0, 9):
        assert p._lib.gpf_regions_set(p._h, 1, K, region_array(*[(1, 0.0, 1.0, whole)] * 9)) == -1
        assert f'1 to 8 regions required, got {K}'.encode() in err()
    assert p._lib.gpf_regions_set(p._h, 0, 1, ok) == -1 and b'every >= 1' in err()
    assert p._lib.gpf_regions_set(p._h, 1, 1, None) == -1 and b'null regions' in err()
    for field in (-1, 5):
        assert p._lib.gpf_regions_set(p._h, 1, 2, region_array((1, 0.0, 1.0, whole), (field, 0.0, 1.0, whole))) == -1
        assert f'region 1: unknown field {field}'.encode() in err()
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0), (0.0, float('nan')), (INF, INF)):
        assert p._lib.gpf_regions_set(p._h, 1, 1, region_array((1, lo, hi, whole))) == -1 and b'region 0: lo < hi required' in err(), (lo, hi)
    for box in ((0, nx, 1, ny), (1, nx + 1, 1, ny), (1, nx, 0, ny), (1, nx, 1, ny + 1), (5, 4, 1, ny), (1, nx, 7, 6)):
        assert p._lib.gpf_regions_set(p._h, 1, 1, region_array((1, 0.0, 1.0, box))) == -1 and b'region 0: box' in err(), box
    assert p._lib.gpf_regions_read(p._h, None, None, 0, None, None) == -5 and b'no regions are armed' in err()
    sums, ints = np.empty((8, 9)), np.zeros((8, 5), dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    assert p._lib.gpf_regions_now(p._h, _lib.as_dp(sums), ints.ctypes.data_as(i64p), 8) == -5 and b'no regions are armed' in err()
    ms = C.c_double(0.)
    assert p._lib.gpf_regions_time(p._h, 2, 1, C.byref(ms)) == -5 and b'mode 1 needs armed regions' in err()
    _lib.check(p._lib.gpf_regions_set(p._h, 1, 2, region_array((1, -INF, INF, whole), (2, -INF, INF, (nx, nx, ny, ny)))))
    assert p._lib.gpf_regions_now(p._h, _lib.as_dp(sums), ints.ctypes.data_as(i64p), 1) == -1 and b'room for 2 regions' in err()
    _lib.check(p._lib.gpf_regions_now(p._h, _lib.as_dp(sums), ints.ctypes.data_as(i64p), 8))
    assert ints[0].tolist() == [nx * ny, 1, nx, 1, ny] and ints[1].tolist() == [1, nx, nx, ny, ny] and np.all(np.isfinite(sums[:2]))
    _lib.check(p._lib.gpf_regions_time(p._h, 2, 1, C.byref(ms)))
    assert ms.value > 0
    _lib.check(p._lib.gpf_regions_clear(p._h))
    # an open stage-wise step
    _lib.check(p._lib.gpf_open_step(p._h))
    assert p._lib.gpf_regions_set(p._h, 1, 1, ok) == -5 and b'stage-wise step is open' in err()
    assert p._lib.gpf_regions_clear(p._h) == -5 and b'stage-wise step is open' in err()
    for i in range(2):
        _lib.check(p._lib.gpf_stage_closures(p._h))
        _lib.check(p._lib.gpf_stage_advance(p._h, i))
    sc = _lib.GpfScalars()
    _lib.check(p._lib.gpf_close_step(p._h, C.byref(sc)))
    p.set_regions([{'field': 'rho'}], 2)            # closed: armed; gpf_close_step itself records nothing
    assert p.regions.step.shape == (0,) and p.regions.p.shape == (0, 1) and p.regions.bbox.shape == (0, 1, 4)
    _lib.check(p._lib.gpf_open_step(p._h))
    for i in range(2):
        _lib.check(p._lib.gpf_stage_closures(p._h))
        _lib.check(p._lib.gpf_stage_advance(p._h, i))
    _lib.check(p._lib.gpf_close_step(p._h, C.byref(sc)))
    have = C.c_int64(-1)
    _lib.check(p._lib.gpf_regions_read(p._h, None, None, 0, None, C.byref(have)))
    assert have.value == 0
    # shear thinning
    t = tp.build(THINNING)
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.set_regions([{'field': 'rho'}])
    with pytest.raises(NotImplementedError, match='shear thinning'):
        t.film_regions()
    assert t._lib.gpf_regions_set(t._h, 1, 1, ok) == -1 and b'shear thinning' in t._lib.gpf_last_error()
    # an elastic gap
    e = tp.build(ELASTIC)
    with pytest.raises(NotImplementedError, match='elastic gap'):
        e.set_regions([{'field': 'rho'}])
    assert e._lib.gpf_regions_set(e._h, 1, 1, ok) == -1 and b'elastic handle' in e._lib.gpf_last_error()
    # surrogate closures
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = quiet(Problem.from_string, SURROGATE)
        with pytest.raises(NotImplementedError, match='surrogate'):
            g.set_regions([{'field': 'rho'}])
        quiet(g._pre_run)
        assert g._lib.gpf_regions_set(g._h, 1, 1, ok) == -1 and b'surrogate' in g._lib.gpf_last_error()
    # an armed member of an ensemble: member and reason named, by the package and by the library
    members = [tp.build(JOURNAL_1D), tp.build(JOURNAL_1D.replace('eps: 0.7', 'eps: 0.5'))]
    members[1].set_regions([{'field': 'rho', 'above': RHO_UP}])
    with pytest.raises(NotImplementedError, match='member 1: regions are armed'):
        Ensemble(members)
    handles = (C.c_void_p * 2)(*[m._h.value for m in members])
    ens = C.c_void_p()
    assert members[0]._lib.gpf_ensemble_create(handles, 2, C.byref(ens)) == -1
    assert b'member 1: regions are armed on it (they cut the batch per member; gpf_regions_clear, or step it alone)' in members[0]._lib.gpf_last_error()
    members[1].clear_regions()
    made = Ensemble(members)
    members[0].set_regions([{'field': 'rho', 'above': RHO_UP}])
    with pytest.raises(NotImplementedError, match='member 0: .*regions are armed'):
        made.step(3)


def run_yaml(out, silent, max_it=12):
    options = (f"options: {{output: {out}, write_freq: 5, use_tstamp: False, silent: {silent}, regions: 3, "
               f"region_list: [{{field: rho, above: {RHO_UP}, name: compressed}}, {{field: p, below: 101325.0, box: [10, 90, 1, 1], name: below_p0}}, "
               f"{{field: jx, above: 0.0}}]}}")
    return JOURNAL_1D.replace("options: {silent: True}", options).replace('max_it: 100000', f'max_it: {max_it}')


def test_run_writes_regions_npz_and_a_restored_problem_rearms(hiplib, tmp_path):
    from gapflow_amd import Problem
    p = quiet(Problem.from_string, run_yaml(tmp_path / 'run', False))
    quiet(p.run)
    f = np.load(os.path.join(p.outdir, 'regions.npz'))
    assert sorted(f.files) == sorted(('step', 'time', 'names', 'cells', 'area', 'bbox') + INTEGRANDS)
    assert f['names'].tolist() == ['compressed', 'below_p0', 'r2'] and f['step'].tolist() == [3, 6, 9, 12]
    assert f['p'].shape == (4, 3) and f['bbox'].shape == (4, 3, 4) and f['cells'].dtype == np.int64
    ref = series_runs('small-1d')['series']                 # the same problem and regions (the third named forward there), every = 1
    for q in INTEGRANDS + ('time', 'area'):
        assert_bitwise(f[q], getattr(ref, q)[[2, 5, 8, 11]], f"run() at stride 3 against the batch at stride 1: {q}")
    for q in INTS:
        assert f[q].tolist() == getattr(ref, q)[[2, 5, 8, 11]].tolist()
    # checkpoints do not carry the series: the restored problem re-arms from its options and records from the restart step
    a = quiet(Problem.from_string, run_yaml(tmp_path / 'unused', True, max_it=1000))
    a._pre_run()
    a._advance(5, honor_stop=False)
    a.save_checkpoint(str(tmp_path / 'c.gpf'))
    a._advance(7, honor_stop=False)
    b = quiet(Problem.from_checkpoint, str(tmp_path / 'c.gpf'))
    assert b.regions.step.shape == (0,) and b.regions.names == ('compressed', 'below_p0', 'r2')
    b._advance(7, honor_stop=False)
    assert a.regions.step.tolist() == [3, 6, 9, 12] and b.regions.step.tolist() == [6, 9, 12]
    for n, x in series_arrays(b.regions):
        assert_bitwise(x, dict(series_arrays(a.regions))[n][1:], f"restored against continued: {n}")
    assert b.regions.cells.tolist() == a.regions.cells[1:].tolist() and b.regions.bbox.tolist() == a.regions.bbox[1:].tolist()
    # regions armed from code do not enter the options and do not survive a restore
    c = make('small-1d')
    c.set_regions(SERIES_REGIONS)
    c._advance(2, honor_stop=False)
    c.save_checkpoint(str(tmp_path / 'd.gpf'))
    assert quiet(Problem.from_checkpoint, str(tmp_path / 'd.gpf')).regions is None
    b.clear_regions()
    assert b.regions is None
