"""The three series of an ensemble -- film integrals, extrema, point probes -- share one store, one install step and one way to
the host (csrc/api_ensemble.inc: EnsembleSeries): armed together on one ensemble they are, bit for bit, what each is when armed
alone; arming one leaves the others' records alone; a set the library refuses leaves what is armed as it was; and an ensemble
with all three armed is destroyed cleanly right after a call.

Members: the neighbouring tests' smallest -- their PAIR for the LDS tier (64 x 1 periodic, 37 x 1 Dirichlet) and the 50 x 50 entry
of their WORKSPACE table.  Every comparison is bit for bit; no tolerance appears."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_ensemble import quiet
from test_gpu_ensemble_extrema import WORKSPACE, assert_same_extrema
from test_gpu_ensemble_integrals import PAIR, ensemble
from test_gpu_ensemble_probes import assert_same_probes
from test_gpu_integrals import assert_same_series

pytestmark = pytest.mark.gpu

CASES = [(t, False) for t in PAIR] + WORKSPACE['50x50'][0]         # lds, lds, workspace
CELLS = [(1, 1), (20, 1)]
ARM = {'integrals': lambda ens: ens.set_integrals(2), 'extrema': lambda ens: ens.set_extrema(3), 'probes': lambda ens: ens.set_probes(CELLS, pressure=True)}
SAME = {'integrals': assert_same_series, 'extrema': assert_same_extrema, 'probes': assert_same_probes}
CALLS = [(3, 0, 4), (2, 5, 1)]


def probes_head(hiplib, ens, member):
    """(return code, records of the last call, step count of the first) of gpf_ensemble_probes_read with no room for records"""
    first, have = C.c_int64(-1), C.c_int64(-1)
    rc = hiplib.gpf_ensemble_probes_read(ens._e, member, None, 0, C.byref(first), C.byref(have))
    return rc, have.value, first.value


def test_three_at_once_equal_each_alone(hiplib):
    both, ps = ensemble(CASES)
    assert both.tiers == ['lds', 'lds', 'workspace']
    for arm in ARM.values():
        arm(both)
    alone = {}
    for name, arm in ARM.items():
        alone[name], _ = ensemble(CASES)
        arm(alone[name])
    for k, counts in enumerate(CALLS):
        before = [p.step for p in ps]
        for ens in [both] + list(alone.values()):
            quiet(ens.step, list(counts))
        for ens in (both, alone['probes']):
            for m, n in enumerate(counts):          # a member that took no step left no record; its first step is still its count + 1
                assert probes_head(hiplib, ens, m) == (0, n, before[m] + 1), f"call {k}, member {m}"
    assert [p.step for p in ps] == [5, 5, 5]
    assert [s.step.tolist() for s in both.integrals] == [[2, 4]] * 3
    assert [s.step.tolist() for s in both.extrema] == [[3]] * 3
    assert [s.step.tolist() for s in both.probes] == [[1, 2, 3, 4, 5]] * 3
    for name in ARM:
        for m in range(len(CASES)):
            SAME[name](getattr(both, name)[m], getattr(alone[name], name)[m], f"{name}, member {m}: armed with the others against armed alone")
    assert all(np.ptp(s.p) > 0 for s in both.probes)


def test_arming_one_leaves_the_others_alone(hiplib):
    ens, ps = ensemble(CASES)
    twin, _ = ensemble(CASES)
    for e in (ens, twin):
        e.set_integrals(2)
        quiet(e.step, 4)
    kept = ens.integrals
    assert [s.step.tolist() for s in kept] == [[2, 4]] * 3
    ens.set_extrema(1)
    assert [s.step.tolist() for s in ens.extrema] == [[]] * 3
    for m in range(3):
        assert_same_series(ens.integrals[m], kept[m], f"member {m}: integrals after set_extrema")
    for e in (ens, twin):
        quiet(e.step, 2)
    assert [s.step.tolist() for s in ens.extrema] == [[5, 6]] * 3
    for m in range(3):                              # the series goes on as if nothing had been armed beside it
        assert ens.integrals[m].step.tolist() == [2, 4, 6]
        assert_same_series(ens.integrals[m], twin.integrals[m], f"member {m}: integrals across set_extrema")


def test_a_refused_set_keeps_what_is_armed(hiplib):
    i32 = C.POINTER(C.c_int32)
    ens, ps = ensemble(CASES)
    have = C.c_int64(-1)
    # integrals at stride 2; an x-section outside member 1's 37 rows
    ens.set_integrals(2)
    quiet(ens.step, 1)
    bad = np.array([1, 40], dtype=np.int32)
    assert hiplib.gpf_ensemble_integrals_set(ens._e, 1, 2, bad.ctypes.data_as(i32), 0, None) == -1
    assert b'member 1: x-section 1 at row 40' in hiplib.gpf_last_error()
    quiet(ens.step, 3)
    assert hiplib.gpf_ensemble_integrals_read(ens._e, 0, None, 0, None, C.byref(have)) == 0 and have.value == 2
    assert [s.step.tolist() for s in ens.integrals] == [[2, 4]] * 3
    # extrema at stride 3; every = 0 through the C entry point
    ens.set_extrema(3)
    quiet(ens.step, 1)
    assert hiplib.gpf_ensemble_extrema_set(ens._e, 0) == -1 and b'every >= 1' in hiplib.gpf_last_error()
    quiet(ens.step, 2)
    assert hiplib.gpf_ensemble_extrema_read(ens._e, 0, None, None, 0, None, C.byref(have)) == 0 and have.value == 1
    assert [s.step.tolist() for s in ens.extrema] == [[6]] * 3
    # probes; 256 cells per member against a budget of 1 MiB
    ens.set_probes(CELLS)
    quiet(ens.step, 1)
    old = os.environ.get('GPF_ENSEMBLE_PROBES_MB')
    os.environ['GPF_ENSEMBLE_PROBES_MB'] = '1'
    try:
        with pytest.raises(Exception, match=r"budget of 1048576 bytes \(GPF_ENSEMBLE_PROBES_MB"):
            ens.set_probes([(1, 1)] * 256)
    finally:
        if old is None:
            del os.environ['GPF_ENSEMBLE_PROBES_MB']
        else:
            os.environ['GPF_ENSEMBLE_PROBES_MB'] = old
    quiet(ens.step, 2)
    assert probes_head(hiplib, ens, 2) == (0, 2, 9)
    assert [s.step.tolist() for s in ens.probes] == [[8, 9, 10]] * 3 and ens.probes[0].rho.shape == (3, 2)
    assert [s.step.tolist() for s in ens.integrals] == [[2, 4, 6, 8, 10]] * 3          # and the other two went on beside them
    assert [s.step.tolist() for s in ens.extrema] == [[6, 9]] * 3


def test_destroy_with_all_three_armed_after_a_call(hiplib):
    ens, ps = ensemble(CASES)
    for arm in ARM.values():
        arm(ens)
    quiet(ens.step, 3)
    assert hiplib.gpf_ensemble_destroy(ens._e) == 0
    ens._e.value = None                             # (Ensemble.__del__ has nothing left to destroy)
    assert [p.step for p in ps] == [3, 3, 3]        # the members are their own
    quiet(ps[0]._advance, 1, honor_stop=False)
    assert ps[0].step == 4
