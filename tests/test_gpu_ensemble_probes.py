"""Point probes of ensembles (gpf_ensemble_probes_*, Ensemble.set_probes / probes): both one-workgroup kernels write a record per
committed step inside the batch, into per-member slots the ensemble owns.

Every comparison is bit for bit (values, steps, times); no tolerance appears.  An LDS-tier member runs the body of k_small_steps,
so its reference is the same problem alone with Problem.set_probes.  A workspace-tier member is bit for bit the same however its
steps are split into calls: a twin ensemble stepped one step per call gives q at the probe cells, and p is held to
models.pressure.eos_pressure of the recorded density -- the device's equation of state, as tests/test_gpu_probes.py obtains it.
The probes include a corner ghost cell, both edge cells and the ghost cells beside them."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_ensemble import assert_bitwise, bits, build, journal, quiet
from test_gpu_ensemble_integrals import PAIR, asperity, ensemble

pytestmark = pytest.mark.gpu

CELLS = [[(0, 0), (0, 1), (1, 1), (30, 1), (64, 1), (65, 1), (65, 2)],          # 64 x 1: ghosted 66 x 3
         [(0, 1), (1, 1), (19, 1), (37, 1), (38, 1)]]                           # 37 x 1: ghosted 39 x 3


def assert_same_probes(got, want, what, pick=None):
    sel = slice(None) if pick is None else list(pick)
    assert type(got) is type(want) and np.array_equal(got.cells, want.cells), what
    assert got.step.tolist() == want.step[sel].tolist(), f"{what}: steps {got.step.tolist()}"
    assert_bitwise(got.time, want.time[sel], f"{what}: time")
    for name in ('rho', 'jx', 'jy', 'p'):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), f"{what}: {name}"
        if a is not None:
            assert_bitwise(a, b[sel], f"{what}: {name}")


_SOLO = {}


def solo_series(m, n, pressure=True):
    """Member m of PAIR alone, set_probes(CELLS[m]), n steps in one gpf_step (k_small_steps): computed once, shared, left unchanged."""
    if (m, n, pressure) not in _SOLO:
        p = build(PAIR[m])
        p.set_probes(CELLS[m], pressure=pressure)
        quiet(p._advance, n, honor_stop=False)
        assert p.step == n
        _SOLO[(m, n, pressure)] = p.probes
    return _SOLO[(m, n, pressure)]


def test_lds_tier_equals_the_solo_series(hiplib):
    """One list of cells per member, 40 steps in one call: values, cells, steps and times are the solo problem's."""
    ens, ps = ensemble([(t, False) for t in PAIR])
    assert ens.tiers == ['lds', 'lds'] and ens.probes is None
    ens.set_probes(CELLS)
    assert [s.rho.shape for s in ens.probes] == [(0, 7), (0, 5)]
    quiet(ens.step, 40)
    for m in range(2):
        want = solo_series(m, 40)
        assert want.step.tolist() == list(range(1, 41)) and np.ptp(want.p) > 0
        assert_same_probes(ens.probes[m], want, f"member {m}")
        assert ps[m].probes is None
        ix, iy = np.array(CELLS[m]).T
        assert_bitwise(ens.probes[m].rho[-1], ps[m].q[0, ix, iy], f"member {m}: last record against q")


def test_uneven_calls_and_one_list_for_all(hiplib):
    """[5, 0], [4, 7], [3, 2] without p: every committed step of each member once, in order; a member given 0 steps keeps its
    series; one list of cells holds for both members."""
    ens, ps = ensemble([(t, False) for t in PAIR])
    cells = [(0, 1), (1, 1), (19, 1), (37, 1), (38, 1)]
    ens.set_probes(cells, pressure=False)
    quiet(ens.step, [5, 0])
    assert [s.step.tolist() for s in ens.probes] == [[1, 2, 3, 4, 5], []]
    have, first = C.c_int64(-1), C.c_int64(-1)
    assert hiplib.gpf_ensemble_probes_read(ens._e, 1, None, 0, C.byref(first), C.byref(have)) == 0 and have.value == 0
    quiet(ens.step, [4, 7])
    assert hiplib.gpf_ensemble_probes_read(ens._e, 0, None, 0, C.byref(first), C.byref(have)) == 0 and (first.value, have.value) == (6, 4)
    quiet(ens.step, [3, 2])
    assert [p.step for p in ps] == [12, 9]
    assert [s.step.tolist() for s in ens.probes] == [list(range(1, 13)), list(range(1, 10))]
    assert all(s.p is None and s.cells.tolist() == [list(c) for c in cells] for s in ens.probes)
    assert_same_probes(ens.probes[1], solo_series(1, 40, False), 'member 1', pick=range(9))
    other = build(PAIR[0])
    other.set_probes(cells, pressure=False)
    quiet(other._advance, 12, honor_stop=False)
    assert_same_probes(ens.probes[0], other.probes, 'member 0')


WORKSPACE = {'50x50': ([(asperity(50, 50), False)], 'auto', [(0, 0), (0, 25), (1, 1), (25, 25), (50, 50), (51, 50), (51, 51), (17, 0)]),
             '64x1-forced': ([(journal(64, mc=1), False)], 'workspace', CELLS[0])}


@pytest.mark.parametrize('name', list(WORKSPACE))
def test_workspace_tier(hiplib, name):
    """12 steps in one call against a twin ensemble stepped one step per call: q at the probe cells after each call, p the
    device's equation of state of the recorded density."""
    from gapflow_amd.models.pressure import eos_pressure
    cases, tier, cells = WORKSPACE[name]
    rec, _ = ensemble(cases, tier)
    assert rec.tiers == ['workspace']
    rec.set_probes(cells)
    quiet(rec.step, 12)
    s = rec.probes[0]
    assert s.step.tolist() == list(range(1, 13)) and s.rho.shape == (12, len(cells))
    twin, ps = ensemble(cases, tier)
    ix, iy = np.array(cells).T
    for k in range(12):
        quiet(twin.step, 1)
        assert bits(s.time[k]) == bits(ps[0].simtime), f"time of step {k + 1}"
        for c, field in enumerate(('rho', 'jx', 'jy')):
            assert_bitwise(getattr(s, field)[k], ps[0].q[c, ix, iy], f"step {k + 1}: {field}")
    want = eos_pressure(s.rho, ps[0].prop)
    print(f"{name}: p against eos_pressure(rho): {int((bits(s.p) != bits(want)).sum())} of {want.size} values differ in their bits, "
          f"largest relative difference {np.max(np.abs(s.p - want) / np.abs(want)):.3e}")
    assert np.all(np.isfinite(s.p)) and np.ptp(s.rho) > 0
    assert_bitwise(s.p, want, 'p against eos_pressure of the recorded density')


def test_stop_and_rollback(hiplib):
    """run() with one member that stops at max_it = 7, one rolled back in its fourth step (an absurd dt: a numerical rollback that
    the step handles) and one that goes its 12 steps: a record for every committed step and none for the rolled-back one."""
    from gapflow_amd import Ensemble
    texts = [journal(64, max_it=7, mc=1), journal(40, adaptive=0, dt='1e-10', max_it=12), journal(72, eps=0.5, max_it=12)]
    cells = [(0, 1), (1, 1), (20, 1), (40, 1), (41, 1)]

    def spoil(p):
        p._lib.gpf_set_dt(p._h, 1.0)
        p.dt = 1.0

    alone = [build(t) for t in texts]
    for p in alone:
        p.set_probes(cells)
        quiet(p._advance, 3, honor_stop=False)
    spoil(alone[1])
    for p in alone:
        quiet(p.run)
    for tier in ('auto', 'workspace'):
        ps = [build(t) for t in texts]
        ens = Ensemble(ps, tier=tier)
        ens.set_probes(cells)
        quiet(ens.step, 3)
        spoil(ps[1])
        quiet(ens.run)
        assert [p.step for p in ps] == [p.step for p in alone] == [7, 3, 12] and ps[1]._stop
        assert [s.step.tolist() for s in ens.probes] == [list(range(1, 8)), [1, 2, 3], list(range(1, 13))]
        ix, iy = np.array(cells).T
        for m, (p, s) in enumerate(zip(ps, alone)):
            if tier == 'auto':
                assert_same_probes(ens.probes[m], s.probes, f"member {m}")
            assert_bitwise(ens.probes[m].rho[-1], p.q[0, ix, iy], f"{tier}, member {m}: last record against q")


def test_arguments_and_lifetime(hiplib):
    ens, ps = ensemble([(t, False) for t in PAIR])
    with pytest.raises(ValueError, match=r"member 1: probes: cell \(64, 1\) \(entry 0\) lies outside the ghosted grid 0\.\.38 x 0\.\.2"):
        ens.set_probes([(64, 1)])
    with pytest.raises(ValueError, match=r"member 0: probes: 257 cells, at most 256"):
        ens.set_probes([(1, 1)] * 257)
    with pytest.raises(ValueError, match='3 lists of cells for 2 members'):
        ens.set_probes([[(1, 1)], [(1, 1)], [(1, 1)]])
    assert ens.probes is None
    # the library's own checks name the member
    i32 = C.POINTER(C.c_int32)

    def raw(counts, cells, per_member=1, pressure=1):
        n, c = np.array(counts, dtype=np.int32), np.array(cells, dtype=np.int32)
        return hiplib.gpf_ensemble_probes_set(ens._e, per_member, n.ctypes.data_as(i32), c.ctypes.data_as(i32), pressure)
    assert raw([1, 1], [(64, 1), (64, 1)]) == -1 and b'member 1: probe 0 at cell (64, 1) lies outside 0..38 x 0..2' in hiplib.gpf_last_error()
    assert raw([257], [(1, 1)] * 257, per_member=0) == -1 and b'member 0: probe 256 is one too many (257 given' in hiplib.gpf_last_error()
    assert raw([1, 0], [(1, 1)]) == -1 and b'member 1: n >= 1 cells required' in hiplib.gpf_last_error()
    have = C.c_int64(0)
    assert hiplib.gpf_ensemble_probes_read(ens._e, 0, None, 0, None, C.byref(have)) == -5           # read before set
    # the budget: 2 members x 4096 records x 5 cells x 4 values x 8 bytes = 1 310 720 bytes > 1 MiB; 4 cells fit
    old = os.environ.get('GPF_ENSEMBLE_PROBES_MB')
    os.environ['GPF_ENSEMBLE_PROBES_MB'] = '1'
    try:
        with pytest.raises(Exception, match=r"need 1310720 bytes .*budget of 1048576 bytes \(GPF_ENSEMBLE_PROBES_MB"):
            ens.set_probes([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1)])
        assert hiplib.gpf_ensemble_probes_read(ens._e, 0, None, 0, None, C.byref(have)) == -5       # a failed set arms nothing
        ens.set_probes([(1, 1), (2, 1), (3, 1), (4, 1)])
    finally:
        if old is None:
            del os.environ['GPF_ENSEMBLE_PROBES_MB']
        else:
            os.environ['GPF_ENSEMBLE_PROBES_MB'] = old
    assert [p.step for p in ps] == [0, 0]
    quiet(ens.step, 4)
    assert [s.step.tolist() for s in ens.probes] == [[1, 2, 3, 4]] * 2
    with pytest.raises(ValueError, match='member 1'):       # a failed set leaves the series as they were
        ens.set_probes([(64, 1)])
    assert [s.step.tolist() for s in ens.probes] == [[1, 2, 3, 4]] * 2
    ens.set_probes(CELLS)                           # set twice: new series
    assert [s.rho.shape for s in ens.probes] == [(0, 7), (0, 5)]
    quiet(ens.step, 1)
    assert [s.step.tolist() for s in ens.probes] == [[5], [5]]
    ens.clear_probes()
    assert ens.probes is None
    assert hiplib.gpf_ensemble_probes_read(ens._e, 0, None, 0, None, C.byref(have)) == -5
    quiet(ens.step, 2)                              # clear, then step: steps on, records nothing
    assert [p.step for p in ps] == [7, 7] and ens.probes is None
    # a member armed on itself is refused as ever, in the existing words
    ps[1].set_probes([(1, 1)])
    with pytest.raises(NotImplementedError, match=r"member 1: probes are armed on it \(their records need per-member slots\)"):
        ens.step(1)


def test_run_writes_probes_npz(hiplib, tmp_path):
    """A non-silent member's series goes to probes.npz when its run ends: the arrays a solo run writes."""
    from gapflow_amd import Ensemble
    opts = [f"output: {tmp_path / name}, write_freq: 100, use_tstamp: False, silent: False" for name in ('ens', 'solo')]
    p, alone = build(journal(64, max_it=6, mc=1, options=opts[0])), build(journal(64, max_it=6, mc=1, options=opts[1]))
    alone.set_probes(CELLS[0])
    quiet(alone.run)
    ens = Ensemble([p])
    ens.set_probes(CELLS[0])
    quiet(ens.run)
    got, want = np.load(tmp_path / 'ens' / 'probes.npz'), np.load(tmp_path / 'solo' / 'probes.npz')
    assert sorted(got.files) == sorted(want.files) == ['cells', 'jx', 'jy', 'p', 'rho', 'step', 'time'] and got['step'].tolist() == list(range(1, 7))
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k
