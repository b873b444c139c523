"""options.extrema: read from the YAML text beside the sanitised dictionaries and checked on the host; the five entry points in
the header and the library; the refusals of SlabProblem and Ensemble -- no GPU (the device side: tests/test_gpu_extrema.py)."""
import ctypes
import io
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('gpf_extrema_set', 'gpf_extrema_clear', 'gpf_extrema_read', 'gpf_extrema_now', 'gpf_extrema_time')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_extrema
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_extrema(d, text)
    return d, before


def test_stride_is_read_from_the_yaml_text():
    d, _ = parsed(", extrema: 5")
    assert d['options']['extrema'] == 5
    d, _ = parsed(", extrema: 0")           # 0: off, like an absent key
    assert d['options']['extrema'] == 0


def test_absent_key_means_unarmed_and_leaves_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and 'extrema' not in d['options']


@pytest.mark.parametrize('bad', ["-1", "-3", "1.5", "True", "[1]", "'often'"])
def test_negative_or_non_integer_stride_raises(bad):
    with pytest.raises(ValueError, match='extrema'):
        parsed(f", extrema: {bad}")


def test_set_extrema_stride_is_checked_on_the_host():
    from gapflow_amd.problem import _extrema_stride
    assert _extrema_stride(3, allow_zero=False) == 3
    for bad in (0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='extrema'):
            _extrema_stride(bad, allow_zero=False)


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
    assert _lib.EXTREMA_NAMES == ('p_max', 'p_min', 'rho_max', 'rho_min', 'h_min', 'u_max', 'v_max')


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='extrema: not available on a SlabProblem'):
        SlabProblem.set_extrema(object(), every=2)
    with pytest.raises(NotImplementedError, match='extrema: not available on a SlabProblem'):
        SlabProblem.field_extrema(object())
    with pytest.raises(NotImplementedError, match='extrema: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", extrema: 4"), device=0, dist=object())


def member(extrema_every):
    """What Ensemble's host-side refusal reads of a Problem, without a device behind it."""
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape = (102, 3)
    p._integral_every, p._probe_cells, p._extrema_every = None, None, extrema_every
    return p


def test_ensemble_names_the_armed_member_and_the_reason():
    from gapflow_amd import Ensemble
    from gapflow_amd.ensemble import _refusal
    assert _refusal(member(None)) is None
    with pytest.raises(NotImplementedError, match=r'member 1: extrema are armed on it .*clear_extrema\(\)'):
        Ensemble([member(None), member(2)])


def test_slab_problem_takes_a_zero_stride_as_off():
    """options.extrema: 0 means off on a SlabProblem as on a Problem: the constructor goes on (and trips over the stand-in for
    the process group, long before any device) instead of refusing extrema."""
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(Exception) as e:
        SlabProblem.from_string(BASE.format(more=", extrema: 0"), device=0, dist=object())
    assert not isinstance(e.value, NotImplementedError) and 'extrema' not in str(e.value)
