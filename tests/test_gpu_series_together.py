"""Every series armed on one handle at once, held bit for bit against the same run with each series armed alone: what one walk
over the series does for one of them (begin, launch, collect, the cuts of a one-workgroup batch, the records that wait for
gpf_elastic_update) must not depend on which others are armed beside it.

Fused steps: the eight series gpf_step records -- probes (every step), film integrals 2, weighted integrals 3, regions 7, lines 5,
extrema 6, statistics 4 with after = 4 (the first record is step 8: a batch is not cut at step 4), changes 3 (the weighted
integrals' stride again) -- over 13 steps as two calls, 6 + 7, so that the second batch begins off the strides 4, 5 and 7 and on
2, 3 and 6.  Grids: 20 x 18 steps through the one-workgroup kernel (the cuts and the in-kernel recorders), 37 x 40 is the
smallest shape of tests/edge_rule_cases.py that takes a launch per step (one partial strip, rows that do not divide into chunks).
Stage-wise steps: an elastic problem on tests/test_gpu_elastic_series.py's smallest grid (48 x 30) with probes, extrema 2, film
integrals 3, the deformation series 1 and statistics 1 with after = 2, over 4 update() calls, each with its gpf_elastic_update.
No tolerance anywhere.  Reference: none (the reference post-processes written frames)."""
import functools

import numpy as np
import pytest

import test_gpu_elastic_series as tes
from test_gpu_probes import DN, build
from test_gpu_series_order import TEXT

pytestmark = pytest.mark.gpu

CALLS = (6, 7)
GRIDS = {'one-workgroup-20x18': (20, 18), 'launch-per-step-37x40': (37, 40)}


def weights(nx, ny):
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    return np.stack([0.5 + ix / nx, np.cos(0.3 * iy) ** 2])


# name -> (arm(p), read(p)): `read` returns the series as the problem hands it out
FUSED = {
    'probes': (lambda p: p.set_probes([(0, 0), (1, 1), (p.grid['Nx'] // 2, 3), (p.grid['Nx'] + 1, p.grid['Ny'] + 1)]), lambda p: p.probes),
    'integrals': (lambda p: p.set_integrals(2), lambda p: p.integrals),
    'weighted': (lambda p: p.set_weighted_integrals(weights(p.grid['Nx'], p.grid['Ny']), 3), lambda p: p.weighted_integrals),
    'regions': (lambda p: p.set_regions([{'field': 'h', 'above': 6.e-6, 'below': 1.e-5}, {'field': 'rho', 'box': [2, 9, 3, 11]}], 7),
                lambda p: p.regions),
    'lines': (lambda p: p.set_lines([{'along': 'x'}, {'along': 'y', 'at': [2, 5]}, {'along': 'x', 'at': [3, 8]}], 5), lambda p: p.lines),
    'extrema': (lambda p: p.set_extrema(6), lambda p: p.extrema),
    'statistics': (lambda p: p.set_statistics(4, after=4), lambda p: p.statistics),
    'changes': (lambda p: p.set_changes(3), lambda p: p.changes),
}
ELASTIC = {
    'probes': (lambda p: p.set_probes([(0, 0), (7, 11), (49, 31)]), lambda p: p.probes),
    'extrema': (lambda p: p.set_extrema(2), lambda p: p.extrema),
    'integrals': (lambda p: p.set_integrals(3), lambda p: p.integrals),
    'elastic_series': (lambda p: p.set_elastic_series(1), lambda p: p.elastic_series),
    'statistics': (lambda p: p.set_statistics(1, after=2), lambda p: p.statistics),
}
# the step counts each series must hold at the end (the statistics: count, first and last step of the window)
FUSED_STEPS = {'probes': list(range(1, 14)), 'integrals': [2, 4, 6, 8, 10, 12], 'weighted': [3, 6, 9, 12], 'regions': [7], 'lines': [5, 10],
               'extrema': [6, 12], 'statistics': (2, 8, 12), 'changes': [3, 6, 9, 12]}
ELASTIC_STEPS = {'probes': [1, 2, 3, 4], 'extrema': [2, 4], 'integrals': [3], 'elastic_series': [1, 2, 3, 4], 'statistics': (2, 3, 4)}


def frozen(x):
    """A series as nested dicts of (dtype, shape, bytes): equal exactly when every array holds the same bits"""
    if x is None:
        return None
    if hasattr(x, '_asdict'):
        x = x._asdict()
    if isinstance(x, dict):
        return {k: frozen(v) for k, v in x.items()}
    a = np.ascontiguousarray(x)
    return (a.dtype.str, a.shape, a.tobytes())


def steps_of(series):
    if isinstance(series, dict) and 'count' in series:
        return (series['count'], series['first_step'], series['last_step'])
    return (series['step'] if isinstance(series, dict) else series.step).tolist()


def fused_run(grid, armed):
    nx, ny = GRIDS[grid]
    p = build(TEXT.format(nx=nx, ny=ny, bc=DN))
    for name in armed:
        FUSED[name][0](p)
    for n in CALLS:
        assert len(p._advance(n, honor_stop=False)) == n
    small = p.integrals_in_batch if 'integrals' in armed else None
    return {name: FUSED[name][1](p) for name in armed}, p.q.copy(), small


def elastic_run(armed):
    p = tes.build(tes.text_of('48x30'))
    for name in armed:
        ELASTIC[name][0](p)
    for _ in range(4):
        p.update()
    assert p.step == 4
    return {name: ELASTIC[name][1](p) for name in armed}, p.q.copy(), None


@functools.lru_cache(maxsize=None)
def runs(case):
    """Per case, computed once and only read: the run with everything armed, and per series the run with it alone"""
    table, run = (ELASTIC, elastic_run) if case == 'elastic' else (FUSED, functools.partial(fused_run, case))
    return run(tuple(table)), {name: run((name,)) for name in table}


def check(case, want_steps):
    (together, q, small), alone = runs(case)
    for name, series in together.items():
        lone, lone_q, _ = alone[name]
        assert steps_of(series) == steps_of(lone[name]) == want_steps[name], f"{case}: {name}: the recorded steps"
        a, b = frozen(series), frozen(lone[name])
        differ = [k for k in a if a[k] != b[k]]
        assert a.keys() == b.keys() and not differ, f"{case}: {name} beside the others against {name} alone: {differ} differ"
        assert q.tobytes() == lone_q.tobytes(), f"{case}: q with everything armed against q with {name} alone"
    return small


@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_fused_series_together_are_each_series_alone(hiplib, grid):
    small = check(grid, FUSED_STEPS)
    assert small is (grid == 'one-workgroup-20x18'), "the grid does not take the step path this case is about"


def test_elastic_series_together_are_each_series_alone(hiplib):
    check('elastic', ELASTIC_STEPS)
