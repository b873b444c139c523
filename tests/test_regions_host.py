"""Region series, host side: options.regions / options.region_list read from the YAML text beside the sanitised dictionaries, the
checks of a region list, the SlabProblem and Ensemble refusals, the C ABI's declarations and the slot arithmetic of a small-grid
batch cut at the union of the armed series' strides -- no GPU and no device call (the device side: tests/test_gpu_regions.py, the
predicate itself: tests/test_regions_hostcheck.py)."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('gpf_regions_set', 'gpf_regions_clear', 'gpf_regions_read', 'gpf_regions_now', 'gpf_regions_time')
INF = float('inf')

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_regions
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_regions(d, text)
    return d, before


def test_region_keys_are_read_from_the_yaml_text():
    d, _ = parsed(", regions: 5, region_list: [{field: rho, below: 850.0, name: cavitated}, {field: p, above: 1.0e+6, box: [1, 64, 1, 3]}, "
                  "{field: h, above: -.inf, below: .inf}]")
    assert d['options']['regions'] == 5
    assert d['options']['region_list'] == [{'field': 'rho', 'above': -INF, 'below': 850.0, 'box': None, 'name': 'cavitated'},
                                           {'field': 'p', 'above': 1.0e6, 'below': INF, 'box': [1, 64, 1, 3], 'name': 'r1'},
                                           {'field': 'h', 'above': -INF, 'below': INF, 'box': None, 'name': 'r2'}]
    d, _ = parsed(", regions: 0")                       # 0: off, and nothing to list
    assert d['options']['regions'] == 0 and 'region_list' not in d['options']


def test_absent_keys_leave_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and 'regions' not in d['options'] and 'region_list' not in d['options']


@pytest.mark.parametrize('bad', ["-3", "1.5", "True", "[1]", "'often'"])
def test_malformed_stride_raises(bad):
    with pytest.raises(ValueError, match='regions: the stride'):
        parsed(f", regions: {bad}, region_list: [{{field: rho}}]")


def test_a_stride_without_a_list_raises():
    with pytest.raises(ValueError, match='options.region_list must list'):
        parsed(", regions: 2")


@pytest.mark.parametrize('bad,entry', [("[{field: q}]", 0), ("[{field: rho}, {below: 3.}]", 1), ("[{field: rho, above: 2., below: 2.}]", 0),
                                       ("[{field: rho, above: 3., below: 2.}]", 0), ("[{field: rho, above: .nan}]", 0),
                                       ("[{field: rho, below: low}]", 0), ("[{field: rho, above: True}]", 0),
                                       ("[{field: h}, {field: p, box: [1, 2, 3]}]", 1), ("[{field: p, box: [0, 5, 1, 6]}]", 0),
                                       ("[{field: p, box: [1, 101, 1, 6]}]", 0), ("[{field: p, box: [1, 100, 1, 7]}]", 0),
                                       ("[{field: p, box: [5, 4, 1, 6]}]", 0), ("[{field: p, box: [1, 5, 4, 3]}]", 0),
                                       ("[{field: p, box: [1, 2.5, 1, 2]}]", 0), ("[{field: jx, nme: x}]", 0), ("[{field: jx, name: 3}]", 0),
                                       ("[{field: jx, name: a}, {field: jy, name: a}]", 1), ("[[rho, 1, 2]]", 0)])
def test_malformed_entries_raise_naming_the_entry(bad, entry):
    with pytest.raises(ValueError, match=rf'options\.region_list: entry {entry}\b'):
        parsed(f", regions: 2, region_list: {bad}")


@pytest.mark.parametrize('bad', ["[]", "7", "{field: rho}", "'all'", "[" + ", ".join(["{field: rho}"] * 9) + "]"])
def test_lists_that_are_no_list_of_1_to_8_raise(bad):
    with pytest.raises(ValueError, match=r'options\.region_list: a list of 1 to 8 regions'):
        parsed(f", regions: 2, region_list: {bad}")


def test_entries_checked_from_code():
    from gapflow_amd.problem import _region_entries
    got = _region_entries([{'field': 'jy', 'above': np.float64(0.0)}, {'field': 'h', 'below': 1, 'box': (2, 2, np.int64(5), 5)}], 7, 5)
    assert got == [{'field': 'jy', 'above': 0.0, 'below': INF, 'box': None, 'name': 'r0'},
                   {'field': 'h', 'above': -INF, 'below': 1.0, 'box': [2, 2, 5, 5], 'name': 'r1'}]
    assert len(_region_entries([{'field': 'rho'}] * 8)) == 8           # 8 is the most; without a grid the upper box edges are not checked
    with pytest.raises(ValueError, match=r'regions: entry 0: box'):
        _region_entries([{'field': 'rho', 'box': [1, 8, 1, 5]}], 7, 5)
    with pytest.raises(ValueError, match=r'regions: entry 0: above < below'):
        _region_entries([{'field': 'rho', 'above': INF}], 7, 5)


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='regions: not available on a SlabProblem'):
        SlabProblem.set_regions(object(), [{'field': 'rho'}], every=2)
    with pytest.raises(NotImplementedError, match='regions: not available on a SlabProblem'):
        SlabProblem.film_regions(object())
    with pytest.raises(NotImplementedError, match='regions: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", regions: 4, region_list: [{field: rho, below: 850.}]"), device=0, dist=object())


def member(regions_every):
    """What Ensemble's host-side refusal reads of a Problem, without a device behind it."""
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p._h = None
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape = (102, 3)
    p._integral_every, p._weighted_every, p._probe_cells, p._extrema_every, p._stats_every = None, None, None, None, None
    p._regions_every = regions_every
    return p


def test_ensemble_names_the_armed_member_and_the_reason():
    from gapflow_amd import Ensemble
    from gapflow_amd.ensemble import _refusal
    assert _refusal(member(None)) is None
    with pytest.raises(NotImplementedError, match=r'member 1: regions are armed on it .*clear_regions\(\)'):
        Ensemble([member(None), member(2)])
    with open(os.path.join(ROOT, 'gapflow_amd', 'csrc', 'api_ensemble.inc')) as f:       # the library's line, as the issue words it
        assert 'regions are armed on it (they cut the batch per member; gpf_regions_clear, or step it alone)' in f.read()


def test_entry_points_are_declared_bound_and_exported():
    from gapflow_amd import _lib
    with open(os.path.join(ROOT, 'include', 'gapflow_hip.h')) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(rf'^int {name}\(gpf_handle\* h', header, re.M), f"{name} is not declared in include/gapflow_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    i64p, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    want = {'gpf_regions_set': ('int64_t every, int K, const gpf_region* regions', [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(_lib.GpfRegion)]),
            'gpf_regions_clear': ('', []),
            'gpf_regions_read': ('double* sums, int64_t* ints, int64_t capacity_records, int64_t* steps_out, int64_t* n_records',
                                 [dp, i64p, ctypes.c_int64, i64p, i64p]),
            'gpf_regions_now': ('double* sums, int64_t* ints, int64_t count', [dp, i64p, ctypes.c_int64]),
            'gpf_regions_time': ('int64_t n, int mode, double* ms', [ctypes.c_int64, ctypes.c_int, dp])}
    for name, (decl, args) in want.items():
        m = re.search(rf'^int {name}\(gpf_handle\* h(.*?)\);', header, re.M)
        got = re.sub(r'/\*.*?\*/', '', m.group(1)).strip().lstrip(',').strip()
        assert got == decl, f"{name}: declared with ({got})"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p] + args), name
    # gpf_region: int32 field, int32 box[4], double lo, hi
    assert re.search(r'int32_t field;.*\n\s*int32_t box\[4\];.*\n\s*double\s+lo, hi;.*\n\} gpf_region;', header)
    assert ctypes.sizeof(_lib.GpfRegion) == 40 and _lib.GpfRegion.lo.offset == 24 and _lib.GpfRegion.hi.offset == 32 and _lib.GpfRegion.box.offset == 4
    for k, f in enumerate(_lib.REGION_FIELDS):
        assert re.search(rf'^#define GPF_REGION_{f.upper()}\s+{k}$', header, re.M), f
    assert _lib.REGION_MAX == 8 and _lib.REGION_INTS == ('cells', 'ix_min', 'ix_max', 'iy_min', 'iy_max')
    if os.path.exists(_lib.LIB_PATH):       # where a built library is present: it exports them (opened, not initialised)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), f"{_lib.LIB_PATH} does not export {name}"


def cuts_model(base, ran, strides):
    """A model of csrc/api_series.inc: small_batch_cut for series that record at the multiples of their strides (0: not armed): the
    step counts at which a small-grid batch over the steps (base, base + ran] is cut.  The C++ itself is held by
    tests/test_gpu_regions.py (series armed together at different strides); this pins the arithmetic it must agree with."""
    end, at, cuts = base + ran, base, []
    while at < end:
        nxt = end
        for every in strides:
            if every:
                nxt = min(nxt, (at // every + 1) * every)
        cuts.append(nxt)
        at = nxt
    return cuts


@pytest.mark.parametrize('strides', [(1, 1, 1), (2, 3, 5), (0, 0, 4), (7, 0, 5), (4, 8, 0), (50, 7, 3), (0, 0, 0), (4096, 3, 2)])
def test_slot_arithmetic_for_the_union_of_three_strides(strides):
    """A small-grid batch is cut at the union of the film integrals', the weighted integrals' and the regions' recorded steps; each
    series keeps the slots of its own stride (the third stride is the regions')."""
    from gapflow_amd.problem import _integral_records
    for base in (0, 1, 5, 6, 7, 49, 50, 4095, 12345):
        for ran in (1, 2, 6, 7, 13, 50, 99):
            cuts = cuts_model(base, ran, strides)
            steps = range(base + 1, base + ran + 1)
            assert cuts == sorted({s for s in steps for e in strides if e and s % e == 0} | {base + ran}), (base, ran, strides)
            assert all(b > a for a, b in zip([base] + cuts, cuts))          # every piece advances
            for every in strides:
                if not every:
                    continue
                recorded = [s for s in cuts if s % every == 0]
                assert recorded == [s for s in steps if s % every == 0]         # no recorded step is skipped by the others' cuts
                for rank, s in enumerate(recorded):
                    assert _integral_records(base, s - base, every) - 1 == rank
                assert _integral_records(base, ran, every) == len(recorded)
    assert cuts_model(3, 0, strides) == []
