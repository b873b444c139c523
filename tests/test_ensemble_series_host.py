"""Host side of the ensembles' extrema series and point probes: declarations, exports, the null-argument refusals (which need no
device) and Ensemble.set_extrema's / set_probes' own validation, on a stub.  No GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {'gpf_ensemble_extrema_set': r'gpf_ensemble\* e, int64_t every',
            'gpf_ensemble_extrema_clear': r'gpf_ensemble\* e',
            'gpf_ensemble_extrema_read': r'gpf_ensemble\* e, int member, double\* values, int32_t\* cells, int64_t capacity_records, int64_t\* steps_out, '
                                         r'int64_t\* n_records',
            'gpf_ensemble_probes_set': r'gpf_ensemble\* e, int per_member, const int32_t\* nprobe, const int32_t\* cells, int with_pressure',
            'gpf_ensemble_probes_clear': r'gpf_ensemble\* e',
            'gpf_ensemble_probes_read': r'gpf_ensemble\* e, int member, double\* out, int64_t capacity_records, int64_t\* first_step, int64_t\* n_records'}
NARGS = {'gpf_ensemble_extrema_set': 2, 'gpf_ensemble_extrema_clear': 1, 'gpf_ensemble_extrema_read': 7, 'gpf_ensemble_probes_set': 5,
         'gpf_ensemble_probes_clear': 1, 'gpf_ensemble_probes_read': 6}


def test_entry_points_are_declared_bound_and_exported():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    with open(os.path.join(ROOT, 'include', 'gapflow_hip.h')) as f:
        header = f.read()
    lib = ctypes.CDLL(build_library())
    for name, args in DECLARED.items():
        assert re.search(rf'^int {name}\({args}\);', header, re.M), f"{name} is not declared in include/gapflow_hip.h"
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == NARGS[name], name
        assert hasattr(lib, name), f"{name} is not exported"
    assert 'GPF_ENSEMBLE_PROBES_MB' in header
    with open(os.path.join(ROOT, 'README.md')) as f:
        assert '| `GPF_ENSEMBLE_PROBES_MB=m` |' in f.read()


def test_null_arguments_are_invalid():
    from gapflow_amd import _lib
    lib = _lib.load()
    n, first = ctypes.c_int64(7), ctypes.c_int64(7)
    one = (ctypes.c_int32 * 2)(1, 1)
    assert lib.gpf_ensemble_extrema_set(None, 1) == -1 and b'gpf_ensemble_extrema_set' in lib.gpf_last_error()
    assert lib.gpf_ensemble_extrema_clear(None) == -1 and b'gpf_ensemble_extrema_clear' in lib.gpf_last_error()
    assert lib.gpf_ensemble_extrema_read(None, 0, None, None, 0, None, ctypes.byref(n)) == -1 and b'gpf_ensemble_extrema_read' in lib.gpf_last_error()
    assert lib.gpf_ensemble_probes_set(None, 0, one, one, 1) == -1 and b'gpf_ensemble_probes_set' in lib.gpf_last_error()
    assert lib.gpf_ensemble_probes_clear(None) == -1 and b'gpf_ensemble_probes_clear' in lib.gpf_last_error()
    assert lib.gpf_ensemble_probes_read(None, 0, None, 0, ctypes.byref(first), ctypes.byref(n)) == -1 and b'gpf_ensemble_probes_read' in lib.gpf_last_error()
    assert (n.value, first.value) == (7, 7)         # nothing was written
    # a null output or input beside a handle that is never looked at before the check
    fake = ctypes.c_void_p(8)
    assert lib.gpf_ensemble_extrema_read(fake, 0, None, None, 0, None, None) == -1
    assert lib.gpf_ensemble_probes_read(fake, 0, None, 0, None, None) == -1
    assert lib.gpf_ensemble_probes_set(fake, 0, None, one, 1) == -1 and lib.gpf_ensemble_probes_set(fake, 0, one, None, 1) == -1


class _NoLibrary:
    def __getattr__(self, name):
        pytest.fail(f"the library was called ({name})")


class _Recorder:
    """Stands in for the library: keeps what gpf_ensemble_probes_set / gpf_ensemble_extrema_set were given."""

    def __init__(self):
        self.calls = []

    def gpf_ensemble_probes_set(self, e, per_member, nprobe, cells, pressure):
        counts = [nprobe[i] for i in range(self.members if per_member else 1)]
        total = sum(counts)
        self.calls.append(('probes', per_member, counts, [(cells[2 * k], cells[2 * k + 1]) for k in range(total)], pressure))
        return 0

    def gpf_ensemble_extrema_set(self, e, every):
        self.calls.append(('extrema', every))
        return 0


def bare(shapes, lib=None):
    """An Ensemble of what set_probes / set_extrema read of its members, without a device."""
    from gapflow_amd import Ensemble
    ens = Ensemble.__new__(Ensemble)
    ens.problems = [SimpleNamespace(grid={'Nx': nx, 'Ny': ny}, _shape=(nx + 2, ny + 2)) for nx, ny in shapes]
    ens._lib, ens._e = lib or _NoLibrary(), None
    ens._integral_every = ens._extrema_every = ens._probe_cells = None
    if lib is not None:
        lib.members = len(shapes)
    return ens


@pytest.mark.parametrize('cells, match', [([(64, 1)], r'member 1: probes: cell \(64, 1\) \(entry 0\) lies outside the ghosted grid 0\.\.38 x 0\.\.2'),
                                          ([(1, 3)], r'member 0: probes: cell \(1, 3\)'),
                                          ([[(1, 1)], [(1, 1), (39, 0)]], r'member 1: probes: cell \(39, 0\) \(entry 1\)'),
                                          ([[(1, 1)], []], r'member 1: probes: at least one cell'),
                                          ([[(1, 1)]], r'1 lists of cells for 2 members'),
                                          ([[(1, 1)], [(1, 1)], [(1, 1)]], r'3 lists of cells for 2 members'),
                                          ([(1, 1)] * 257, r'member 0: probes: 257 cells, at most 256'),
                                          ([(1, 1.0)], r'member 0: probes: entry 0 must be a pair of integers'),
                                          ([], r'member 0: probes: at least one cell'),
                                          ('11', r'member 0: probes: a list of \[ix, iy\] cells is required')])
def test_set_probes_validates_on_the_host(cells, match):
    ens = bare([(64, 1), (37, 1)])
    with pytest.raises(ValueError, match=match):
        ens.set_probes(cells)
    assert ens.probes is None


def test_set_probes_passes_one_list_or_one_per_member():
    lib = _Recorder()
    ens = bare([(64, 1), (37, 1)], lib)
    ens.set_probes([(0, 0), (38, 2)], pressure=False)
    assert lib.calls[-1] == ('probes', 0, [2], [(0, 0), (38, 2)], 0)
    assert [s.cells.tolist() for s in ens.probes] == [[[0, 0], [38, 2]]] * 2 and all(s.p is None and s.rho.shape == (0, 2) for s in ens.probes)
    ens.set_probes([[(65, 2)], np.array([[1, 1], [38, 0]])])
    assert lib.calls[-1] == ('probes', 1, [1, 2], [(65, 2), (1, 1), (38, 0)], 1)
    assert [s.cells.tolist() for s in ens.probes] == [[[65, 2]], [[1, 1], [38, 0]]] and ens.probes[1].p.shape == (0, 2)


@pytest.mark.parametrize('every', [0, -1, True, 2.0, None])
def test_set_extrema_validates_the_stride_on_the_host(every):
    ens = bare([(64, 1)])
    with pytest.raises(ValueError, match='stride'):
        ens.set_extrema(every)
    assert ens.extrema is None


def test_series_are_none_until_armed():
    lib = _Recorder()
    ens = bare([(64, 1), (37, 1)], lib)
    assert ens.extrema is None and ens.probes is None
    ens.clear_extrema(), ens.clear_probes()         # not armed: no library call
    assert lib.calls == []
    ens.set_extrema(3)
    assert lib.calls == [('extrema', 3)]
    assert [type(s).__name__ for s in ens.extrema] == ['FieldExtrema'] * 2 and ens.extrema[0].cells.shape == (0, 7, 2)
    assert ens.integrals is None and ens.probes is None
