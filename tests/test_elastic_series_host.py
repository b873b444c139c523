"""options.elastic_series: read from the YAML text beside the sanitised dictionaries and checked on the host; the five entry points
in the header and the library with the signatures the loader holds; the refusals of SlabProblem and Ensemble; and the record's
definition restated in NumPy -- no GPU (the device side: tests/test_gpu_elastic_series.py)."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARATIONS = {
    'gpf_elastic_series_set': 'gpf_handle* h, int64_t every',
    'gpf_elastic_series_clear': 'gpf_handle* h',
    'gpf_elastic_series_read': 'gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records',
    'gpf_elastic_series_now': 'gpf_handle* h, double values[6], int32_t cells[4]',
    'gpf_elastic_series_time': 'gpf_handle* h, int64_t n, int mode, double* ms',
}

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_elastic_series
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_elastic_series(d, text)
    return d, before


def test_stride_is_read_from_the_yaml_text_and_zero_means_off():
    d, _ = parsed(", elastic_series: 5")
    assert d['options']['elastic_series'] == 5
    d, _ = parsed(", elastic_series: 0")
    assert d['options']['elastic_series'] == 0 and not d['options'].get('elastic_series')      # what Problem.__init__ asks
    d, before = parsed("")
    assert d == before and 'elastic_series' not in d['options']


@pytest.mark.parametrize('bad', ["-1", "1.5", "True", "[1]", "'often'"])
def test_negative_or_non_integer_stride_raises(bad):
    with pytest.raises(ValueError, match='elastic series'):
        parsed(f", elastic_series: {bad}")


def test_set_elastic_series_stride_is_checked_on_the_host():
    from gapflow_amd.problem import _elastic_series_stride
    assert _elastic_series_stride(3, allow_zero=False) == 3
    for bad in (0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='elastic series'):
            _elastic_series_stride(bad, allow_zero=False)


def test_header_declares_the_entry_points_and_the_library_exports_them():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    text = open(os.path.join(ROOT, 'include', 'gapflow_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(build_library())
    ctype_of = {'gpf_handle*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'double*': _lib._DP,
                'int32_t*': ctypes.POINTER(ctypes.c_int32), 'int64_t*': ctypes.POINTER(ctypes.c_int64)}
    for name, args in DECLARATIONS.items():
        assert re.search(rf'^int {name}\({re.escape(args)}\);', text, re.M), f'{name}({args}) is not declared in include/gapflow_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        restype, argtypes = _lib.SIGNATURES[name]
        want = []
        for a in args.split(', '):
            kind, ident = a.rsplit(' ', 1)
            want.append(ctype_of[kind + '*' if ident.endswith(']') else kind])       # (an array parameter is a pointer)
        assert restype is ctypes.c_int and argtypes == want, name
    assert _lib.ELASTIC_SERIES_NAMES == ('d_sum', 'd2_sum', 'p_d', 'h_sum', 'd_max', 'd_min')


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='elastic series: not available on a SlabProblem'):
        SlabProblem.set_elastic_series(object(), every=2)
    with pytest.raises(NotImplementedError, match='elastic series: not available on a SlabProblem'):
        SlabProblem.film_elastic(object())
    with pytest.raises(NotImplementedError, match='elastic series: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", elastic_series: 4"), device=0, dist=object())
    with pytest.raises(Exception) as e:         # 0: off, as on a Problem -- the constructor goes on to the stand-in process group
        SlabProblem.from_string(BASE.format(more=", elastic_series: 0"), device=0, dist=object())
    assert not isinstance(e.value, NotImplementedError) and 'elastic series' not in str(e.value)


def test_problem_without_an_elastic_gap_refuses_on_the_host():
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._elastic = None
    with pytest.raises(NotImplementedError, match='no elastic gap'):
        p.set_elastic_series(1)
    with pytest.raises(NotImplementedError, match='no elastic gap'):
        p.film_elastic()


def test_ensemble_refuses_a_member_with_an_elastic_gap():
    """The only problems that can arm the series are elastic, and those an Ensemble does not take."""
    from gapflow_amd import Ensemble, Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, object()
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=True)
    p._shape = (102, 3)
    p._integral_every, p._probe_cells, p._extrema_every, p._elastic_series_every = None, None, None, 2
    with pytest.raises(NotImplementedError, match='member 0: an elastic gap'):
        Ensemble([p])


# ---------------------------------------------------------------------------------------------------------------------------
# the record's definition, restated: the pair walk, the fold trees, the one comparison
# ---------------------------------------------------------------------------------------------------------------------------
def block_sum(vals):
    """series_rows.hpp: block_sum of 256 threads' values -- lanes 32, 16, .. 1 apart, then waves 0..3 in order to +0.0."""
    out = np.float64(0.0)
    for w in range(4):
        lane = [np.float64(v) for v in vals[64 * w:64 * w + 64]]
        for s in (32, 16, 8, 4, 2, 1):
            lane = [lane[i] + (lane[i + s] if i + s < 64 else lane[i]) for i in range(64)]     # (__shfl_down past the wave: own value; lane 0 never reads one)
        out = out + lane[0]
    return out


def tree_sum(term):
    """Sum of an interior plane [Nx][Ny] in the device's order: per row, thread t adds the pairs (2k, 2k + 1), k = t, t + 256, ...,
    the lower column first; block_sum; over the rows thread t adds rows t, t + 256, ...; block_sum."""
    nx, ny = term.shape
    rows = []
    for ix in range(nx):
        th = [np.float64(0.0)] * 256
        for k in range((ny + 1) // 2):
            for iy in (2 * k, 2 * k + 1):
                if iy < ny:
                    th[k % 256] = th[k % 256] + term[ix, iy]
        rows.append(block_sum(th))
    th = [np.float64(0.0)] * 256
    for ix in range(nx):
        th[ix % 256] = th[ix % 256] + rows[ix]
    return block_sum(th)


def before(want_min, a, ax, ay, b, bx, by):
    """series_first.hpp: extrema_before."""
    if a != b:
        return a < b if want_min else a > b
    return ax < bx if ax != bx else ay < by


def first(d, want_min, order):
    """The first candidate under `before`, visiting the interior cells in `order`: any order gives the same cell."""
    best = None
    for ix, iy in order:
        c = (d[ix, iy], ix + 1, iy + 1)
        if best is None or before(want_min, *c, *best):
            best = c
    return best


def test_record_definition_on_a_small_plane_with_ties_and_a_negative_zero():
    """5 x 4 interior: the maximum 2.0 sits at three cells, the minimum is a tie of -0.0 and +0.0 (equal under IEEE: the smaller
    ix, then the smaller iy wins whichever sign it carries)."""
    d = np.array([[1.0, 0.5, 2.0, 1.5],
                  [0.0, 2.0, 1.0, 0.25],
                  [1.0, -0.0, 0.5, 2.0],
                  [0.75, 1.0, 0.0, 1.0],
                  [1.0, 1.0, 1.0, 1.0]])
    cells = [(ix, iy) for ix in range(5) for iy in range(4)]
    rng = np.random.default_rng(5)
    for order in (cells, cells[::-1], [cells[k] for k in rng.permutation(len(cells))]):
        assert first(d, False, order) == (2.0, 1, 3)
        got = first(d, True, order)
        assert got[1:] == (2, 1) and got[0] == 0.0 and not np.signbit(got[0])
    # np.argmax / np.argmin over the C-ordered interior is the same tie rule
    assert divmod(int(np.argmax(d)), 4) == (0, 2) and divmod(int(np.argmin(d)), 4) == (1, 0)
    # the sums: the device's tree against fsum, within the rounding of its depth; zeros stay +0.0
    p = 1.0e5 + 1.0e3 * rng.random(d.shape)
    for term in (d, d * d, p * d):
        exact = float(np.sum([float(x) for x in term.ravel()]))
        assert abs(tree_sum(term) - exact) <= 24 * 2.0 ** -53 * np.abs(term).sum()
    z = tree_sum(np.zeros((5, 4)) * p)
    assert z == 0.0 and not np.signbit(z)
    assert not np.signbit(tree_sum(np.full((5, 4), -0.0)))         # a set that starts at +0.0 is never -0.0
