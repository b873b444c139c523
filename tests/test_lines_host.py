"""Line profiles, host side: options.lines / options.line_list read from the YAML text beside the sanitised dictionaries, the checks
of a line list and of set_lines' arguments, the default centre indices against ny // 2 / nx // 2 of the ghosted shape, the
SlabProblem and Ensemble refusals, the C ABI's declarations and what the five entry points return for a null handle and null
arguments -- no GPU and no device call (the device side: tests/test_gpu_lines.py, the index arithmetic itself:
tests/test_lines_hostcheck.py)."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('gpf_lines_set', 'gpf_lines_clear', 'gpf_lines_read', 'gpf_lines_now', 'gpf_lines_time')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_lines
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_lines(d, text)
    return d, before


def test_line_keys_are_read_from_the_yaml_text():
    d, _ = parsed(", lines: 5, line_list: [{along: x}, {along: y, at: [1, 32], name: band}, {along: x, at: 6}]")
    assert d['options']['lines'] == 5
    assert d['options']['line_list'] == [{'along': 'x', 'at': None, 'name': 'l0'}, {'along': 'y', 'at': [1, 32], 'name': 'band'},
                                         {'along': 'x', 'at': 6, 'name': 'l2'}]
    d, _ = parsed(", lines: 0")                         # 0: off, and nothing to list
    assert d['options']['lines'] == 0 and 'line_list' not in d['options']


def test_absent_keys_leave_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and 'lines' not in d['options'] and 'line_list' not in d['options']


@pytest.mark.parametrize('bad', ["-3", "1.5", "True", "[1]", "'often'"])
def test_malformed_stride_raises(bad):
    with pytest.raises(ValueError, match='lines: the stride'):
        parsed(f", lines: {bad}, line_list: [{{along: x}}]")


def test_a_stride_without_a_list_raises():
    with pytest.raises(ValueError, match='options.line_list must list'):
        parsed(", lines: 2")


@pytest.mark.parametrize('bad,entry', [("[{along: z}]", 0), ("[{along: x}, {at: 3}]", 1), ("[{along: x, at: 0}]", 0), ("[{along: x, at: 7}]", 0),
                                       ("[{along: y, at: 101}]", 0), ("[{along: x, at: [4, 3]}]", 0), ("[{along: x, at: [1, 7]}]", 0),
                                       ("[{along: x}, {along: y, at: [0, 5]}]", 1), ("[{along: y, at: [1, 2, 3]}]", 0), ("[{along: x, at: 2.5}]", 0),
                                       ("[{along: x, at: True}]", 0), ("[{along: x, at: mid}]", 0), ("[{along: x, nme: a}]", 0),
                                       ("[{along: x, name: 3}]", 0), ("[{along: x, name: step}]", 0), ("[{along: x, name: a}, {along: y, name: a}]", 1),
                                       ("[[x, 1]]", 0)])
def test_malformed_entries_raise_naming_the_entry(bad, entry):
    with pytest.raises(ValueError, match=rf'options\.line_list: entry {entry}\b'):
        parsed(f", lines: 2, line_list: {bad}")


@pytest.mark.parametrize('bad', ["[]", "7", "{along: x}", "'all'", "[" + ", ".join(["{along: x}"] * 9) + "]"])
def test_lists_that_are_no_list_of_1_to_8_raise(bad):
    with pytest.raises(ValueError, match=r'options\.line_list: a list of 1 to 8 lines'):
        parsed(f", lines: 2, line_list: {bad}")


def test_entries_checked_from_code():
    from gapflow_amd.problem import _line_entries, _line_span
    got = _line_entries([{'along': 'y', 'at': np.int64(7)}, {'along': 'x', 'at': (2, np.int32(5)), 'name': 'band'}, {'along': 'x'}], 7, 5)
    assert got == [{'along': 'y', 'at': 7, 'name': 'l0'}, {'along': 'x', 'at': [2, 5], 'name': 'band'}, {'along': 'x', 'at': None, 'name': 'l2'}]
    assert [_line_span(e, 7, 5) for e in got] == [(7, 7), (2, 5), (3, 3)]
    assert len(_line_entries([{'along': 'x'}] * 8)) == 8            # 8 is the most; without a grid the upper index is not checked
    assert _line_entries([{'along': 'x', 'at': 10 ** 6}])[0]['at'] == 10 ** 6
    with pytest.raises(ValueError, match=r'lines: entry 0: at must be first <= last inside'):
        _line_entries([{'along': 'x', 'at': 6}], 7, 5)                 # along x the index is a column: 1..Ny
    assert _line_entries([{'along': 'y', 'at': 6}], 7, 5)[0]['at'] == 6     # along y a row: 1..Nx
    with pytest.raises(ValueError, match=r'lines: entry 1: the name'):
        _line_entries([{'along': 'x'}, {'along': 'y', 'name': 'l0'}], 7, 5)


@pytest.mark.parametrize('nx,ny', [(45, 37), (20, 70), (100, 1), (1, 1), (2, 2), (3, 8), (4096, 4096), (7, 1)])
def test_default_centre_is_the_references_centre_line_of_the_ghosted_frame(nx, ny):
    """viz/plotting.py draws field[1:-1, ny // 2] and field[nx // 2, 1:-1] with (nx, ny) the GHOSTED shape: the default `at` is that
    column / row as an interior index, and it is an interior cell."""
    from gapflow_amd.problem import _line_centre, _line_span
    frame = np.arange((nx + 2) * (ny + 2)).reshape(nx + 2, ny + 2)
    gx, gy = frame.shape
    cx, cy = _line_centre('x', nx, ny), _line_centre('y', nx, ny)
    assert cx == gy // 2 and cy == gx // 2 and 1 <= cx <= ny and 1 <= cy <= nx
    assert frame[1:-1, cx].tolist() == frame[1:-1, gy // 2].tolist() and frame[cy, 1:-1].tolist() == frame[gx // 2, 1:-1].tolist()
    assert _line_span({'along': 'x', 'at': None}, nx, ny) == (cx, cx) and _line_span({'along': 'y', 'at': None}, nx, ny) == (cy, cy)
    if ny == 1:
        assert cx == 1


def bare(lines_every=None):
    """What set_lines' own checks and Ensemble's host-side refusal read of a Problem, without a device behind it."""
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape = (102, 3)
    p.grid = {'Nx': 100, 'Ny': 1}
    p._integral_every, p._weighted_every, p._probe_cells, p._extrema_every, p._stats_every, p._regions_every = None, None, None, None, None, None
    p._lines_every = lines_every
    return p


def test_argument_validation_happens_before_any_library_call():
    """Every refusal below is raised with `_lib` and `_h` absent: an AttributeError would show a call that got past the checks."""
    p = bare()
    ok = [{'along': 'x'}]
    with pytest.raises(ValueError, match='a list of 1 to 8 lines'):
        p.set_lines([{'along': 'x'}] * 9)
    with pytest.raises(ValueError, match='a list of 1 to 8 lines'):
        p.set_lines([])
    with pytest.raises(ValueError, match='entry 0: along must be one of'):
        p.set_lines([{'along': 'z'}])
    with pytest.raises(ValueError, match='entry 0: at must be first <= last inside'):
        p.set_lines([{'along': 'x', 'at': 2}])                      # Ny = 1
    with pytest.raises(ValueError, match='entry 0: at must be first <= last inside'):
        p.set_lines([{'along': 'y', 'at': (5, 4)}])
    with pytest.raises(ValueError, match='entry 0: at must be first <= last inside'):
        p.set_lines([{'along': 'y', 'at': (1, 101)}])
    with pytest.raises(ValueError, match='entry 1: the name'):
        p.set_lines([{'along': 'x', 'name': 'a'}, {'along': 'y', 'name': 'a'}])
    for every in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match='lines: the stride'):
            p.set_lines(ok, every)
    for capacity in (0, -4, 2.0, True):
        with pytest.raises(ValueError, match='lines: capacity'):
            p.set_lines(ok, 1, capacity)
    assert p.lines is None
    with pytest.raises(RuntimeError, match='no lines are set'):
        p.film_lines()
    with pytest.raises(ValueError, match='a list of 1 to 8 lines'):
        p.film_lines(lines=[])
    p.clear_lines()                                                 # nothing armed: nothing to call
    for attr, why in (('has_gp_model', 'surrogate'), ('_elastic', 'elastic gap')):
        q = bare()
        setattr(q, attr, True)
        with pytest.raises(NotImplementedError, match=f'lines: .*{why}'):
            q.set_lines(ok)
        with pytest.raises(NotImplementedError, match=f'lines: .*{why}'):
            q.film_lines(ok)
    q = bare()
    q._cfg.thinning = 1
    with pytest.raises(NotImplementedError, match='lines: shear thinning'):
        q.set_lines(ok)


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='lines: not available on a SlabProblem'):
        SlabProblem.set_lines(object(), [{'along': 'x'}], every=2)
    with pytest.raises(NotImplementedError, match='lines: not available on a SlabProblem'):
        SlabProblem.film_lines(object())
    with pytest.raises(NotImplementedError, match='lines: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", lines: 4, line_list: [{along: x}]"), device=0, dist=object())
    with pytest.raises(Exception) as e:         # 0: off, as on a Problem -- the constructor goes on and trips over the stand-in group
        SlabProblem.from_string(BASE.format(more=", lines: 0"), device=0, dist=object())
    assert not isinstance(e.value, NotImplementedError) and 'lines' not in str(e.value)


def test_ensemble_names_the_armed_member_and_the_reason():
    from gapflow_amd import Ensemble
    from gapflow_amd.ensemble import _refusal
    assert _refusal(bare(None)) is None
    with pytest.raises(NotImplementedError, match=r'member 1: lines are armed on it .*clear_lines\(\)'):
        Ensemble([bare(None), bare(2)])
    with open(os.path.join(ROOT, 'gapflow_amd', 'csrc', 'api_ensemble.inc')) as f:       # the library's line
        assert 'lines are armed on it (they cut the batch per member; gpf_lines_clear, or step it alone)' in f.read()


def test_entry_points_are_declared_and_bound():
    from gapflow_amd import _lib
    with open(os.path.join(ROOT, 'include', 'gapflow_hip.h')) as f:
        header = f.read()
    i64p, dp, lp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_lib.GpfLine)
    want = {'gpf_lines_set': ('int64_t every, int K, const gpf_line* lines , int64_t capacity', [ctypes.c_int64, ctypes.c_int, lp, ctypes.c_int64]),
            'gpf_lines_clear': ('', []),
            'gpf_lines_read': ('double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records', [dp, ctypes.c_int64, i64p, i64p]),
            'gpf_lines_now': ('int K, const gpf_line* lines , double* out, int64_t count', [ctypes.c_int, lp, dp, ctypes.c_int64]),
            'gpf_lines_time': ('int64_t n, int mode, double* ms', [ctypes.c_int64, ctypes.c_int, dp])}
    assert sorted(want) == sorted(ENTRY_POINTS)
    for name, (decl, args) in want.items():
        m = re.search(rf'^int {name}\(gpf_handle\* h(.*?)\);', header, re.M)
        assert m, f"{name} is not declared in include/gapflow_hip.h"
        got = re.sub(r'/\*.*?\*/', '', m.group(1)).strip().lstrip(',').strip()
        assert got == decl, f"{name}: declared with ({got})"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p] + args), name
    # gpf_line: int32 along, int32 i0, i1; the header cites the reference lines the feature serves
    assert re.search(r'int32_t along;.*\n\s*int32_t i0, i1;.*\n\} gpf_line;', header)
    assert ctypes.sizeof(_lib.GpfLine) == 12 and _lib.GpfLine.i0.offset == 4 and _lib.GpfLine.i1.offset == 8
    for k, axis in enumerate(_lib.LINE_AXES):
        assert re.search(rf'^#define GPF_LINE_{axis.upper()} {k}$', header, re.M), axis
    assert 'viz/plotting.py:51-60' in header and 'viz/animations.py:200-242' in header
    assert _lib.LINE_MAX == 8
    assert _lib.LINE_FIELDS == ('rho', 'jx', 'jy', 'p', 'h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')


def test_null_handle_and_null_arguments_are_refused_without_a_device():
    """The library is opened, not initialised: these returns come before anything touches a device.  -1: GPF_ERR_INVALID."""
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    lib = ctypes.CDLL(build_library())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f'{name} is not exported'
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.gpf_last_error.restype = ctypes.c_char_p
    line = (_lib.GpfLine * 1)()
    out, ms, have = np.zeros(9), ctypes.c_double(-1.0), ctypes.c_int64(-7)
    assert lib.gpf_lines_set(None, 1, 1, line, 0) == -1 and b'null handle' in lib.gpf_last_error()
    assert lib.gpf_lines_clear(None) == -1 and b'null handle' in lib.gpf_last_error()
    assert lib.gpf_lines_read(None, _lib.as_dp(out), 1, None, ctypes.byref(have)) == -1 and b'null handle' in lib.gpf_last_error()
    assert have.value == -7 and not out.any()
    assert lib.gpf_lines_now(None, 1, line, _lib.as_dp(out), 9) == -1 and b'gpf_lines_now: null argument' in lib.gpf_last_error()
    assert lib.gpf_lines_time(None, 1, 0, ctypes.byref(ms)) == -1 and b'gpf_lines_time: null argument' in lib.gpf_last_error()
    assert ms.value == -1.0
    # a handle that is not null with the output missing: refused on the argument, before the handle is read
    fake = ctypes.c_void_p(8)
    assert lib.gpf_lines_now(fake, 1, line, None, 9) == -1 and b'gpf_lines_now: null argument' in lib.gpf_last_error()
    assert lib.gpf_lines_time(fake, 1, 0, None) == -1 and b'gpf_lines_time: null argument' in lib.gpf_last_error()
