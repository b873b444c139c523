"""Weighted film integrals, host side: gapflow_amd/weights.py (box / mode / load), options.weighted_integrals / options.weights read
from the YAML text beside the sanitised dictionaries, the SlabProblem refusals, the C ABI's declarations and the slot arithmetic
of a small-grid batch cut at the union of two strides -- no GPU and no device call (the device side: tests/test_gpu_weighted.py)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {'Nx': 7, 'Ny': 5, 'dx': 0.5, 'dy': 0.25}
ENTRY_POINTS = ('gpf_weighted_set', 'gpf_weighted_clear', 'gpf_weighted_read', 'gpf_weighted_now', 'gpf_weighted_time')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more, base_dir=None):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_weighted
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_weighted(d, text, base_dir)
    return d, before


def test_box_is_exactly_zero_or_one_on_inclusive_ranges():
    from gapflow_amd import weights
    w = weights.box(GRID, 2, 4, 5, 5)
    assert w.shape == (7, 5) and w.dtype == np.float64
    want = np.zeros((7, 5))
    want[1:4, 4] = 1.0                      # interior rows 2, 3, 4 and column 5, 1-based and inclusive
    assert w.tobytes() == want.tobytes() and set(np.unique(w)) == {0.0, 1.0}
    assert weights.box(GRID, 1, 7, 1, 5).tobytes() == np.ones((7, 5)).tobytes()
    one = weights.box(GRID, 7, 7, 1, 1)
    assert one.sum() == 1.0 and one[6, 0] == 1.0
    # two boxes that share no cell and leave none out add up to ones
    assert (weights.box(GRID, 1, 3, 1, 5) + weights.box(GRID, 4, 7, 1, 5)).tobytes() == np.ones((7, 5)).tobytes()
    for bad in ((0, 3, 1, 5), (1, 8, 1, 5), (3, 2, 1, 5), (1, 7, 0, 5), (1, 7, 1, 6), (1, 7, 4, 3)):
        with pytest.raises(ValueError, match='box'):
            weights.box(GRID, *bad)
    with pytest.raises(ValueError, match='integer'):
        weights.box(GRID, 1.5, 3, 1, 5)


def test_mode_is_evaluated_at_the_cell_centres():
    from gapflow_amd import weights
    c, s = weights.mode(GRID, 2, 1), weights.mode(GRID, 2, 1, 'sin')
    assert c.shape == s.shape == (7, 5)
    Lx, Ly = 7 * 0.5, 5 * 0.25
    for ix in (1, 4, 7):
        for iy in (1, 5):
            arg = 2 * np.pi * (2 * (ix - 0.5) * 0.5 / Lx + (iy - 0.5) * 0.25 / Ly)
            assert c[ix - 1, iy - 1] == pytest.approx(np.cos(arg), abs=1e-15)
            assert s[ix - 1, iy - 1] == pytest.approx(np.sin(arg), abs=1e-15)
    assert weights.mode(GRID, 0, 0).tobytes() == np.ones((7, 5)).tobytes()
    assert abs(c.sum()) < 1e-13 and abs(s.sum()) < 1e-13 and c.min() < 0 < c.max()       # a whole period: sign-changing, mean zero
    assert np.allclose(c * c + s * s, 1.0, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='phase'):
        weights.mode(GRID, 1, 0, 'tan')


def test_load_reads_npy_planes(tmp_path):
    from gapflow_amd import weights
    a = np.arange(35, dtype=np.float32).reshape(7, 5)
    np.save(tmp_path / 'one.npy', a)
    got = weights.load(tmp_path / 'one.npy')
    assert got.dtype == np.float64 and got.shape == (7, 5) and np.array_equal(got, a)
    np.save(tmp_path / 'two.npy', np.stack([a, 2 * a]))
    assert weights.load(str(tmp_path / 'two.npy')).shape == (2, 7, 5)
    np.save(tmp_path / 'flat.npy', np.arange(5.))
    with pytest.raises(ValueError, match='shape'):
        weights.load(tmp_path / 'flat.npy')
    planes, names = weights.from_entries(GRID, [{'box': [1, 2, 1, 5], 'name': 'pad0'}, {'file': str(tmp_path / 'two.npy'), 'name': 'f'},
                                                {'mode': [1, 0, 'sin'], 'name': 'm'}])
    assert planes.shape == (4, 7, 5) and names == ['pad0', 'f_0', 'f_1', 'm']
    assert planes[0].tobytes() == weights.box(GRID, 1, 2, 1, 5).tobytes() and planes[3].tobytes() == weights.mode(GRID, 1, 0, 'sin').tobytes()
    with pytest.raises(ValueError, match=r'entry 0: .*shape \(7, 5\), the grid is \(3, 5\)'):
        weights.from_entries(dict(GRID, Nx=3), [{'file': str(tmp_path / 'one.npy'), 'name': 'f'}])


def test_weighted_keys_are_read_from_the_yaml_text(tmp_path):
    d, _ = parsed(", weighted_integrals: 5, weights: [{box: [1, 50, 1, 6], name: pad0}, {mode: [2, 0, cos]}, {mode: [1, 1]}, {file: w.npy}]",
                  base_dir=str(tmp_path))
    assert d['options']['weighted_integrals'] == 5
    assert d['options']['weights'] == [{'box': [1, 50, 1, 6], 'name': 'pad0'}, {'mode': [2, 0, 'cos'], 'name': 'w1'},
                                       {'mode': [1, 1, 'cos'], 'name': 'w2'}, {'file': os.path.join(str(tmp_path), 'w.npy'), 'name': 'w3'}]
    d, _ = parsed(", weighted_integrals: 0")            # 0: off, and nothing to list
    assert d['options']['weighted_integrals'] == 0 and 'weights' not in d['options']


def test_absent_keys_leave_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and 'weighted_integrals' not in d['options'] and 'weights' not in d['options']


@pytest.mark.parametrize('bad', ["-3", "1.5", "True", "[1]", "'often'"])
def test_malformed_stride_raises(bad):
    with pytest.raises(ValueError, match='weighted integrals: the stride'):
        parsed(f", weighted_integrals: {bad}, weights: [{{mode: [1, 0]}}]")


def test_a_stride_without_weights_raises():
    with pytest.raises(ValueError, match='options.weights must list'):
        parsed(", weighted_integrals: 2")


@pytest.mark.parametrize('bad,entry', [("[{box: [1, 2, 3]}]", 0), ("[{mode: [1, 0]}, {box: [1, 101, 1, 6]}]", 1), ("[{box: [0, 5, 1, 6]}]", 0),
                                       ("[{mode: [1, 0, tan]}]", 0), ("[{mode: [1.5, 0]}]", 0), ("[{mode: [1, 0]}, {}, {mode: [1, 1]}]", 1),
                                       ("[{box: [1, 2, 1, 2], mode: [1, 0]}]", 0), ("[{file: 7}]", 0), ("[{mode: [1, 0], nme: x}]", 0),
                                       ("[{mode: [1, 0], name: 3}]", 0), ("[[1, 2, 3, 4]]", 0), ("[{box: [1, 2, 1, True]}]", 0)])
def test_malformed_weight_entries_raise_naming_the_entry(bad, entry):
    with pytest.raises(ValueError, match=rf'options\.weights: entry {entry}\b'):
        parsed(f", weighted_integrals: 2, weights: {bad}")


@pytest.mark.parametrize('bad', ["[]", "7", "{box: [1, 2, 1, 2]}", "'all'"])
def test_weights_that_are_no_list_raise(bad):
    with pytest.raises(ValueError, match='options.weights'):
        parsed(f", weighted_integrals: 2, weights: {bad}")


def test_plane_validation_on_the_host():
    from gapflow_amd.problem import _weight_planes
    planes, names = _weight_planes(np.ones((7, 5)), None, 7, 5)
    assert planes.shape == (1, 7, 5) and names == ['w0']
    planes, names = _weight_planes([np.ones((7, 5)), np.zeros((7, 5))], ['a', 'b'], 7, 5)
    assert planes.shape == (2, 7, 5) and names == ['a', 'b']
    for shape in ((5, 7), (1, 9, 7), (7,), (2, 2, 7, 5)):
        with pytest.raises(ValueError, match=r'\(K, 7, 5\)'):
            _weight_planes(np.ones(shape), None, 7, 5)
    with pytest.raises(ValueError, match='0 weight planes, 1 to 8 required'):
        _weight_planes(np.ones((0, 7, 5)), None, 7, 5)
    with pytest.raises(ValueError, match='9 weight planes, 1 to 8 required'):
        _weight_planes(np.ones((9, 7, 5)), None, 7, 5)
    w = np.ones((3, 7, 5))
    w[2, 3, 4] = np.nan
    with pytest.raises(ValueError, match=r'weight plane 2 is not finite at cell \(4, 5\)'):
        _weight_planes(w, None, 7, 5)
    w[2, 3, 4] = np.inf
    with pytest.raises(ValueError, match=r'weight plane 2 is not finite at cell \(4, 5\)'):
        _weight_planes(w, None, 7, 5)
    for names in (['a'], ['a', 'a', 'b'], 'abc', ['a', '', 'c'], ['a', 2, 'c']):
        with pytest.raises(ValueError, match='names'):
            _weight_planes(np.ones((3, 7, 5)), names, 7, 5)


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='weighted integrals: not available on a SlabProblem'):
        SlabProblem.set_weighted_integrals(object(), np.ones((100, 6)), every=2)
    with pytest.raises(NotImplementedError, match='weighted integrals: not available on a SlabProblem'):
        SlabProblem.film_weighted(object())
    with pytest.raises(NotImplementedError, match='weighted integrals: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", weighted_integrals: 4, weights: [{mode: [1, 0]}]"), device=0, dist=object())


def test_entry_points_are_declared_bound_and_exported():
    from gapflow_amd import _lib
    with open(os.path.join(ROOT, 'include', 'gapflow_hip.h')) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(rf'^int {name}\(gpf_handle\* h', header, re.M), f"{name} is not declared in include/gapflow_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert _lib.SIGNATURES['gpf_weighted_set'][1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    assert len(_lib.WEIGHTED_INTEGRANDS) == 9 and _lib.WEIGHTED_INTEGRANDS[:5] == ('p', 'h', 'rho_h', 'jx_h', 'jy_h')
    assert _lib.WEIGHTED_INTEGRANDS[5:] == _lib.INTEGRAL_SUMS[5:]          # the four wall stresses, in the integrals' order
    if os.path.exists(_lib.LIB_PATH):       # where a built library is present: it exports them (opened, not initialised)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), f"{_lib.LIB_PATH} does not export {name}"


def cuts_model(base, ran, every_a, every_b):
    """A model of csrc/api_series.inc: small_batch_cut's next cut applied until the batch's end -- the step counts at which a small-grid
    batch over the steps (base, base + ran] is cut when two series record at strides `every_a` and `every_b` (0: not armed).  The
    C++ itself is held by tests/test_gpu_weighted.py (series armed together at different strides); this pins the arithmetic it
    must agree with: shared cuts, and for each series the slots of its OWN stride (gapflow_amd.problem._integral_records)."""
    end, at, cuts = base + ran, base, []
    while at < end:
        nxt = end
        for every in (every_a, every_b):
            if every:
                nxt = min(nxt, (at // every + 1) * every)
        cuts.append(nxt)
        at = nxt
    return cuts


@pytest.mark.parametrize('ea,eb', [(1, 1), (2, 3), (3, 2), (7, 5), (4, 8), (50, 7), (6, 0), (0, 6), (4096, 3)])
def test_slot_arithmetic_for_the_union_of_two_strides(ea, eb):
    """A small-grid batch is cut at the union of both series' recorded steps; each series keeps the slots of its own stride."""
    from gapflow_amd.problem import _integral_records
    for base in (0, 1, 5, 6, 7, 49, 50, 4095, 12345):
        for ran in (1, 2, 6, 7, 13, 50, 99):
            cuts = cuts_model(base, ran, ea, eb)
            steps = range(base + 1, base + ran + 1)
            union = sorted({s for s in steps for e in (ea, eb) if e and s % e == 0} | {base + ran})
            assert cuts == union, (base, ran, ea, eb)
            assert all(b > a for a, b in zip([base] + cuts, cuts))          # every piece advances
            for every in (ea, eb):
                if not every:
                    continue
                recorded = [s for s in cuts if s % every == 0]
                assert recorded == [s for s in steps if s % every == 0]         # no recorded step is skipped by the other's cuts
                for rank, s in enumerate(recorded):
                    assert _integral_records(base, s - base, every) - 1 == rank
    assert cuts_model(3, 0, ea, eb) == []
