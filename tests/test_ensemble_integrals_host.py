"""Host side of the ensembles' film-integral series and of in-batch recording: declarations, exports, the null-argument
refusals (which need no device) and Ensemble.set_integrals' own validation.  No GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {'gpf_ensemble_integrals_set': r'gpf_ensemble\* e, int64_t every, int nsx, const int32_t\* ix, int nsy, const int32_t\* iy',
            'gpf_ensemble_integrals_clear': r'gpf_ensemble\* e',
            'gpf_ensemble_integrals_read': r'gpf_ensemble\* e, int member, double\* out, int64_t capacity_records, int64_t\* steps_out, int64_t\* n_records',
            'gpf_integrals_in_batch': r'gpf_handle\* h, int\* yes'}


def test_entry_points_are_declared_bound_and_exported():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    with open(os.path.join(ROOT, 'include', 'gapflow_hip.h')) as f:
        header = f.read()
    lib = ctypes.CDLL(build_library())
    for name, args in DECLARED.items():
        assert re.search(rf'^int {name}\({args}\);', header, re.M), f"{name} is not declared in include/gapflow_hip.h"
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
    assert len(_lib.SIGNATURES['gpf_ensemble_integrals_set'][1]) == 6 and len(_lib.SIGNATURES['gpf_ensemble_integrals_read'][1]) == 6


def test_null_arguments_are_invalid():
    from gapflow_amd import _lib
    lib = _lib.load()
    n, yes = ctypes.c_int64(7), ctypes.c_int(7)
    assert lib.gpf_ensemble_integrals_set(None, 1, 0, None, 0, None) == -1 and b'gpf_ensemble_integrals_set' in lib.gpf_last_error()
    assert lib.gpf_ensemble_integrals_clear(None) == -1 and b'gpf_ensemble_integrals_clear' in lib.gpf_last_error()
    assert lib.gpf_ensemble_integrals_read(None, 0, None, 0, None, ctypes.byref(n)) == -1 and b'gpf_ensemble_integrals_read' in lib.gpf_last_error()
    assert lib.gpf_integrals_in_batch(None, ctypes.byref(yes)) == -1 and b'gpf_integrals_in_batch' in lib.gpf_last_error()
    assert (n.value, yes.value) == (7, 7)           # nothing was written
    # a null output beside a handle that is never looked at before the check
    fake = ctypes.c_void_p(8)
    assert lib.gpf_integrals_in_batch(fake, None) == -1
    assert lib.gpf_ensemble_integrals_read(fake, 0, None, 0, None, None) == -1


class _NoLibrary:
    def __getattr__(self, name):
        pytest.fail(f"the library was called ({name})")


def bare(shapes):
    """An Ensemble of what set_integrals reads of its members, without a device."""
    from gapflow_amd import Ensemble
    ens = Ensemble.__new__(Ensemble)
    ens.problems = [SimpleNamespace(grid={'Nx': nx, 'Ny': ny}) for nx, ny in shapes]
    ens._lib, ens._e, ens._integral_every = _NoLibrary(), None, None
    return ens


@pytest.mark.parametrize('kwargs, match', [(dict(every=0), 'stride'), (dict(every=True), 'stride'), (dict(every=2.0), 'stride'),
                                           (dict(sections_x=[1, 40]), r'member 1: .*sections_x\[1\] = 40'),
                                           (dict(sections_y=[2]), r'member 0: .*sections_y\[0\] = 2'),
                                           (dict(sections_x=[0]), r'member 0: .*sections_x\[0\] = 0'),
                                           (dict(sections_x='1'), r'member 0: .*list of interior indices'),
                                           (dict(sections_x=list(range(1, 10))), r'member 0: .*9 sections'),
                                           (dict(sections_y=[1.0]), r'member 0: .*must be an integer')])
def test_set_integrals_validates_on_the_host(kwargs, match):
    ens = bare([(64, 1), (37, 1)])
    with pytest.raises(ValueError, match=match):
        ens.set_integrals(**kwargs)
    assert ens.integrals is None


def test_integrals_are_none_until_armed():
    ens = bare([(64, 1)])
    assert ens.integrals is None
    ens.clear_integrals()                           # not armed: no library call
    assert ens.integrals is None
