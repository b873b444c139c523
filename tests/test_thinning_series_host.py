"""options.thinning_series: read from the YAML text beside the sanitised dictionaries and checked on the host; the five entry
points in the header and the library with the signatures the loader holds; the table row; the refusals that need no device;
and, for every case of tests/thinning_series_cases.py, the two conditions that keep the device test's tolerance from hiding a
wrong stencil -- no GPU (the device side: tests/test_gpu_thinning_series.py)."""
import ctypes
import inspect
import io
import math
import os
import re

import numpy as np
import pytest

import thinning_series_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARATIONS = {
    'gpf_thinning_series_set': 'gpf_handle* h, int64_t every',
    'gpf_thinning_series_clear': 'gpf_handle* h',
    'gpf_thinning_series_read': 'gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records',
    'gpf_thinning_series_now': 'gpf_handle* h, double values[14], int32_t cells[6]',
    'gpf_thinning_series_time': 'gpf_handle* h, int64_t n, int mode, double* ms',
}


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_own_options
    text = tc.BASE.replace('silent: True', 'silent: True' + more)
    assert text != tc.BASE or not more
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_own_options(d, text)
    return d, before


def test_stride_survives_keep_own_options_and_zero_means_off():
    from gapflow_amd import problem
    assert problem._own_thinning_series in problem._OWN_KEYS
    d, _ = parsed(", thinning_series: 5")
    assert d['options']['thinning_series'] == 5
    d, _ = parsed(", thinning_series: 0")
    assert d['options']['thinning_series'] == 0 and not d['options'].get('thinning_series')     # what Problem.__init__ asks
    d, _ = parsed("")
    assert 'thinning_series' not in d['options']


@pytest.mark.parametrize('bad', ["-1", "1.5", "True", "[1]", "'often'"])
def test_negative_or_non_integer_stride_raises(bad):
    with pytest.raises(ValueError, match='thinning series'):
        parsed(f", thinning_series: {bad}")


def test_set_thinning_series_stride_is_checked_on_the_host():
    from gapflow_amd.series import _thinning_series_stride
    assert _thinning_series_stride(3, allow_zero=False) == 3 and _thinning_series_stride(0) == 0
    for bad in (0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='thinning series'):
            _thinning_series_stride(bad, allow_zero=False)


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


def test_names_namedtuple_and_table_row():
    from gapflow_amd import Problem, _lib
    from gapflow_amd.problem import ThinningSeries
    from gapflow_amd.series import ALL_SERIES, SERIES, SERIES_MORE, SERIES_STAGEWISE
    assert _lib.THINNING_SERIES_NAMES == tc.NAMES and len(_lib.THINNING_SERIES_NAMES) == 14
    assert _lib.THINNING_SERIES_EXTREMA == _lib.THINNING_SERIES_NAMES[11:] == tc.EXTREMA
    assert ThinningSeries._fields == ('step', 'time') + _lib.THINNING_SERIES_NAMES + ('cells',)
    # the tables the tests of the series before pin stay what they were; the new row stands behind them
    assert ALL_SERIES == SERIES + SERIES_MORE and [r.marker for r in SERIES_MORE] == ['_frames_every', '_changes_every']
    (row,) = SERIES_STAGEWISE
    assert (row.marker, row.recorder, row.collect, row.write) == ('_thinning_series_every', '_thinning_series_rec', '_collect_thinning_series',
                                                                  '_write_thinning_series')
    assert (row.noun, row.clear, row.refusal, row.fused) == ('thinning series', 'clear_thinning_series', None, False)
    assert "self._thinning_series_every = None" in inspect.getsource(Problem.__init__)
    for name in (row.collect, row.write, row.clear, 'set_thinning_series', 'film_thinning'):
        assert callable(getattr(Problem, name))
    assert isinstance(Problem.thinning_series, property)
    for method in ('_pre_run', '_post_run'):
        assert 'SERIES_STAGEWISE' in inspect.getsource(getattr(Problem, method)), f"Problem.{method} does not walk the new row"
    assert '_collect_thinning_series' in inspect.getsource(Problem._update_with_surrogates)


def test_refusals_that_need_no_device():
    import types
    from gapflow_amd import Problem
    from gapflow_amd.slab import SlabProblem
    for call in (lambda: SlabProblem.set_thinning_series(object(), every=2), lambda: SlabProblem.film_thinning(object())):
        with pytest.raises(NotImplementedError, match='thinning series: not available on a SlabProblem'):
            call()
    p = Problem.__new__(Problem)
    p._cfg, p._gp_models = types.SimpleNamespace(thinning=0), {}
    for call in (lambda: p.set_thinning_series(1), p.film_thinning):
        with pytest.raises(NotImplementedError, match='no shear thinning'):
            call()
    p._cfg, p._gp_models = types.SimpleNamespace(thinning=1), {'xz': object()}
    for call in (lambda: p.set_thinning_series(1), p.film_thinning):
        with pytest.raises(NotImplementedError, match='surrogates'):
            call()
    p._thinning_series_every = None
    assert p.thinning_series is None
    p.clear_thinning_series()           # nothing armed: no library call


def test_sign_pattern_separates_the_cells_of_every_central_difference():
    s = tc.sign_pattern((9, 11))
    assert set(np.unique(s)) == {-1., 1.}
    assert np.all(s[2:, :] == -s[:-2, :]) and np.all(s[:, 2:] == -s[:, :-2])


@pytest.mark.parametrize('name', tc.CASE_NAMES)
def test_the_tolerance_cannot_hide_a_wrong_stencil(name):
    """For the case's initial state and the oracle-stepped one:
    (a) the conditioning allowance stays below 1e-6 sum|term| dA for every quantity;
    (b) in every tau_*, eta_sum and rate_sum the oracle's value moves by at least 1e3 x the tolerance when grad p is set to zero,
        when the two axes are exchanged (2-D cases; thinning_series_cases.terms says what that means under hypot) and when each
        difference is shifted by one cell -- one change at a time;
    (c) the oracle with s = rho * (1 / rho0), the device's form of Dowson-Higginson's s = rho / rho0, stays within a tenth of the
        tolerance in every sum and of the per-cell bound at every extremum: the relative 1e-12 the tolerance grants the device's
        pressure does cover it in these states (thinning_series_cases says where it would not)."""
    o = tc.build_oracle(name)
    steps = tc.CASES[name][1]
    two_d = o.grid['Ny'] > 1
    for state in ('initial', 'stepped'):
        if state == 'stepped':
            for _ in range(steps):
                o.update()
            assert o.step == steps and o.q_is_valid
        ref = tc.oracle_record_of(o)
        for n in tc.SUMS:
            assert ref['allowance'][n] < 1e-6 * ref['magnitude'][n], (name, state, n, ref['allowance'][n] / ref['magnitude'][n])
        # (c) the premise of the tolerance: the device's way to form s = rho / rho0 stays within a tenth of it
        dev = tc.device_form_terms(o.q, o.topo[:3], o.extra[0], o.prop, o.geo, o.grid)
        dA = o.grid['dx'] * o.grid['dy']
        for n in tc.SUMS:
            moved = abs(math.fsum(dev[n].ravel()) * dA - ref['value'][n])
            assert moved <= 0.1 * ref['tol'][n], (name, state, n, moved / ref['tol'][n])
        for f, pick in (('eta', np.argmin), ('eta', np.argmax), ('rate', np.argmax)):
            at = np.unravel_index(int(pick(ref[f])), ref[f].shape)
            moved = abs(dev[f][at] - ref[f][at])
            assert moved <= 0.1 * ref[f + '_bound'][at], (name, state, f, pick.__name__, moved / ref[f + '_bound'][at])
        least = {}
        for stencil in ('zero', 'swap', 'shift') if two_d else ('zero', 'shift'):
            wrong = tc.oracle_record_of(o, stencil)
            for n in tc.GRADIENT_SUMS:
                if not two_d and n in ('tau_yz_bot', 'tau_yz_top') and ref['magnitude'][n] == 0.:
                    continue            # (V = jy = 0 in a 1-D case would leave no yz stress at all; these cases have V != 0)
                least[(stencil, n)] = abs(wrong['value'][n] - ref['value'][n]) / ref['tol'][n]
        print(f"\n[{name}, {state}] least |wrong stencil - right| / tolerance: {min(least.values()):.3e} at {min(least, key=least.get)}; "
              f"largest allowance / magnitude {max(ref['allowance'][n] / ref['magnitude'][n] for n in tc.SUMS):.3e}")
        bad = {k: v for k, v in least.items() if not v >= 1e3}
        assert not bad, f"{name}, {state}: a wrong stencil moves these by less than 1e3 tolerances: {bad}"
