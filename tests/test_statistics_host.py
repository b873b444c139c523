"""options.statistics / statistics_fields / statistics_after: read from the YAML text beside the sanitised dictionaries and checked
on the host; the rank arithmetic of a record; the NumPy restatement of the recurrences against NumPy's own statistics; the five
entry points in the header and the library; the refusals of SlabProblem and Ensemble -- no GPU (the device side:
tests/test_gpu_statistics.py)."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

import statistics_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('gpf_stats_set', 'gpf_stats_clear', 'gpf_stats_info', 'gpf_stats_read', 'gpf_stats_time')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_statistics
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_statistics(d, text)
    return d, before


def test_keys_are_read_from_the_yaml_text():
    d, _ = parsed(", statistics: 5, statistics_fields: [rho, p], statistics_after: 40")
    assert d['options']['statistics'] == 5 and d['options']['statistics_after'] == 40
    assert d['options']['statistics_fields'] == ['p', 'rho']          # the library's order
    d, _ = parsed(", statistics: 0")        # 0: off, like an absent key
    assert d['options']['statistics'] == 0 and 'statistics_fields' not in d['options']


def test_absent_keys_leave_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and not any(k.startswith('statistics') for k in d['options'])


@pytest.mark.parametrize('bad', ["-1", "1.5", "True", "[1]", "'often'"])
def test_malformed_stride_raises_naming_the_key(bad):
    with pytest.raises(ValueError, match=r'statistics: statistics must be an integer'):
        parsed(f", statistics: {bad}")


@pytest.mark.parametrize('bad', ["[]", "p", "[p, p]", "[h]", "[p, 3]", "{p: 1}", "4"])
def test_malformed_fields_raise_naming_the_key(bad):
    with pytest.raises(ValueError, match='statistics_fields'):
        parsed(f", statistics: 2, statistics_fields: {bad}")


@pytest.mark.parametrize('bad', ["-1", "2.5", "False", "[3]", "'late'"])
def test_malformed_after_raises_naming_the_key(bad):
    with pytest.raises(ValueError, match='statistics_after'):
        parsed(f", statistics: 2, statistics_after: {bad}")


def test_set_statistics_arguments_are_checked_on_the_host():
    from gapflow_amd.problem import _statistics_fields, _statistics_stride
    assert _statistics_stride(3, 'statistics', low=1) == 3 and _statistics_stride(0, 'statistics_after', low=0) == 0
    for bad in (0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='statistics'):
            _statistics_stride(bad, 'statistics', low=1)
    assert _statistics_fields(('jy', 'p')) == ('p', 'jy') and _statistics_fields(['rho']) == ('rho',)


@pytest.mark.parametrize('every', [1, 2, 3, 7, 50, 4096])
def test_rank_of_a_record_against_a_brute_force_count(every):
    """n(expect) = expect / every - a / every with a = max(step count at arming, after): the number of recorded steps up to and
    including `expect`, counted by the three conditions themselves."""
    for arm_step in (0, 1, 2, 5, 49, 50, 51, 4095, 4096, 9000):
        for after in (0, 1, 3, 6, 50, 99, 4096, 10000):
            last = max(arm_step, after) + 3 * every + 2
            steps = sc.recorded_steps(1, last, every, arm_step, after)
            assert all(s % every == 0 and s > max(arm_step, after) for s in steps)
            seen = 0
            for expect in range(max(1, max(arm_step, after) - every - 1), last + 1):
                n = sc.rank(expect, every, arm_step, after)
                if expect in steps:
                    seen += 1
                    assert n == steps.index(expect) + 1, (expect, every, arm_step, after)
                else:
                    assert n is None
            assert seen == len(steps) >= 3


def test_rank_matches_the_librarys_source():
    """The C++ the model restates: stats_rank and stats_floor of csrc/api_stats.inc, as written."""
    text = open(os.path.join(ROOT, 'gapflow_amd', 'csrc', 'api_stats.inc')).read()
    assert 'return expect / every - floor / every;' in text
    assert 'return std::max(h->stats.arm_step, h->stats.after);' in text
    assert 'expect % every != 0 || expect <= stats_floor(h)' in text


@pytest.mark.parametrize('seed,shape,nsamples,offset', [(1, (7, 5), 1, 0.), (2, (7, 5), 2, 0.), (3, (13, 9), 40, 0.), (4, (6, 11), 300, 100.)])
def test_restatement_against_numpys_own_statistics(seed, shape, nsamples, offset):
    """The yardstick itself: mean, population variance, min and max of random sequences at 1e-12 relative (the mean relative to the
    largest |x|) -- also for data that sit at 100 with fluctuations of order one, where a sum of squares would lose four digits.
    (An offset of 1e5 would say nothing at this bound: there the samples themselves are rounded at 1.5e-11, which np.var sees too.)"""
    rng = np.random.default_rng(seed)
    x = offset + rng.standard_normal((nsamples,) + shape)
    w = sc.welford(list(x))
    assert w['count'] == nsamples
    scale = max(np.abs(x).max(), 1.0)
    np.testing.assert_allclose(w['mean'], x.mean(axis=0), rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(w['var'], x.var(axis=0), rtol=1e-12, atol=1e-12 * max(x.var(axis=0).max(), 1e-300))
    assert np.array_equal(w['min'], x.min(axis=0)) and np.array_equal(w['max'], x.max(axis=0))
    if nsamples == 1:
        assert not w['m2'].any() and not w['var'].any()


def test_header_declares_the_entry_points_and_the_library_exports_them():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    text = open(os.path.join(ROOT, 'include', 'gapflow_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(build_library())
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(gpf_handle\* h', text), f'{name} is not declared in include/gapflow_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES['gpf_stats_set'][1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    assert _lib.STATS_FIELDS == ('p', 'rho', 'jx', 'jy') and _lib.STATS_QUANTITIES == sc.QUANTITIES


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='statistics: not available on a SlabProblem'):
        SlabProblem.set_statistics(object(), every=2)
    with pytest.raises(NotImplementedError, match='statistics: not available on a SlabProblem'):
        SlabProblem.statistics.fget(object())
    with pytest.raises(NotImplementedError, match='statistics: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", statistics: 4"), device=0, dist=object())
    with pytest.raises(Exception) as e:         # 0: off, as on a Problem -- the constructor goes on and trips over the stand-in group
        SlabProblem.from_string(BASE.format(more=", statistics: 0"), device=0, dist=object())
    assert not isinstance(e.value, NotImplementedError) and 'statistics' not in str(e.value)


def member(stats_every):
    """What Ensemble's host-side refusal reads of a Problem, without a device behind it."""
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape = (102, 3)
    p._integral_every, p._weighted_every, p._probe_cells, p._extrema_every, p._stats_every = None, None, None, None, stats_every
    return p


def test_ensemble_names_the_armed_member_and_the_reason():
    from gapflow_amd import Ensemble
    from gapflow_amd.ensemble import _refusal
    assert _refusal(member(None)) is None
    with pytest.raises(NotImplementedError, match=r'member 1: statistics are armed on it .*clear_statistics\(\)'):
        Ensemble([member(None), member(2)])
