"""options.changes: read from the YAML text beside the sanitised dictionaries and checked on the host; the five entry points in
the header, the library and _lib; the series table; the refusals of SlabProblem and Ensemble -- no GPU (the device side:
tests/test_gpu_changes.py)."""
import ctypes
import inspect
import io
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('gpf_changes_set', 'gpf_changes_clear', 'gpf_changes_read', 'gpf_changes_now', 'gpf_changes_time')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more, keep='_keep_changes'):
    from gapflow_amd import problem
    from gapflow_amd.io import read_yaml_input
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    getattr(problem, keep)(d, text)
    return d, before


@pytest.mark.parametrize('keep', ['_keep_changes', '_keep_own_options'])
def test_stride_is_read_from_the_yaml_text(keep):
    d, _ = parsed(", changes: 5", keep)
    assert d['options']['changes'] == 5
    d, _ = parsed(", changes: 0", keep)         # 0: off, like an absent key
    assert d['options']['changes'] == 0


def test_absent_key_means_unarmed_and_leaves_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and 'changes' not in d['options']


@pytest.mark.parametrize('bad', ["-1", "-3", "1.5", "True", "[1]", "'often'"])
def test_negative_or_non_integer_stride_raises(bad):
    with pytest.raises(ValueError, match='changes'):
        parsed(f", changes: {bad}")


def test_set_changes_stride_is_checked_on_the_host():
    from gapflow_amd.series import _changes_stride
    assert _changes_stride(3, allow_zero=False) == 3 and _changes_stride(0) == 0
    for bad in (0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='changes: the stride must be an integer >= 1'):
            _changes_stride(bad, allow_zero=False)


def test_header_declares_the_entry_points_and_the_library_exports_them():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    text = open(os.path.join(ROOT, 'include', 'gapflow_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(build_library())
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), f'{name} is not declared in include/gapflow_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES['gpf_changes_read'] == _lib.SIGNATURES['gpf_extrema_read']
    assert _lib.SIGNATURES['gpf_changes_now'] == _lib.SIGNATURES['gpf_extrema_now']
    assert _lib.CHANGE_NAMES == ('d2_rho', 'd2_jx', 'd2_jy', 'q2_rho', 'q2_jx', 'q2_jy', 'dmass', 'dmax_rho', 'dmax_jx', 'dmax_jy', 'dt')
    assert _lib.CHANGE_MAXIMA == _lib.CHANGE_NAMES[7:10]


def test_the_table_ends_with_the_new_row_and_series_is_what_it_was():
    from gapflow_amd import Problem
    from gapflow_amd.series import ALL_SERIES, SERIES, SERIES_MORE
    assert [r.marker for r in SERIES] == ['_probe_cells', '_integral_every', '_weighted_every', '_regions_every', '_lines_every',
                                          '_extrema_every', '_elastic_series_every', '_stats_every']
    assert ALL_SERIES == SERIES + SERIES_MORE and ALL_SERIES[:len(SERIES)] == SERIES
    row = ALL_SERIES[-1]
    assert (row.marker, row.recorder, row.collect, row.write) == ('_changes_every', '_changes_rec', '_collect_changes', '_write_changes')
    assert (row.noun, row.clear, row.fused) == ('changes', 'clear_changes', True)
    assert row.refusal[1] == "they cut the batch per member" and row.refusal[0] > max(r.refusal[0] for r in SERIES if r.refusal)
    assert "self._changes_every = None" in inspect.getsource(Problem.__init__)
    for name in (row.collect, row.write, row.clear, 'set_changes', 'step_change'):
        assert callable(getattr(Problem, name))
    assert isinstance(Problem.changes, property)
    for method in ('_pre_run', '_absorb_batch', '_post_run'):
        assert 'ALL_SERIES' in inspect.getsource(getattr(Problem, method)), f"Problem.{method} does not walk the concatenation"


def member(changes_every, **armed):
    """What Ensemble's host-side refusal reads of a Problem, without a device behind it."""
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape, p.grid = (102, 3), {'Nx': 100, 'Ny': 1}
    p._integral_every, p._probe_cells, p._extrema_every, p._changes_every = None, None, None, changes_every
    for k, v in armed.items():
        setattr(p, k, v)
    return p


def test_ensemble_names_the_armed_member_and_the_reason(monkeypatch):
    from gapflow_amd import Ensemble
    from gapflow_amd.ensemble import _refusal
    monkeypatch.delenv('GPF_SMALL_GRID', raising=False)
    assert _refusal(member(None)) is None
    assert _refusal(member(2)) == (NotImplementedError,
                                   "changes are armed on it (they cut the batch per member): clear_changes(), or run it alone")
    with pytest.raises(NotImplementedError, match=r'member 1: changes are armed on it .*clear_changes\(\)'):
        Ensemble([member(None), member(2)])
    # behind every other series in the order of the refusals
    assert _refusal(member(2, _extrema_every=1))[1].startswith('extrema are armed')


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='changes: not available on a SlabProblem'):
        SlabProblem.set_changes(object(), every=2)
    with pytest.raises(NotImplementedError, match='changes: not available on a SlabProblem'):
        SlabProblem.step_change(object())
    with pytest.raises(NotImplementedError, match='changes: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", changes: 4"), device=0, dist=object())
    # 0 means off on a SlabProblem as on a Problem: the constructor goes on (and trips over the stand-in for the process group,
    # long before any device) instead of refusing changes
    with pytest.raises(Exception) as e:
        SlabProblem.from_string(BASE.format(more=", changes: 0"), device=0, dist=object())
    assert not isinstance(e.value, NotImplementedError) and 'changes' not in str(e.value)
