"""Film-integral series of ensembles (gpf_ensemble_integrals_*, Ensemble.set_integrals / integrals): both one-workgroup kernels
write the record inside the batch (csrc/integral_kernels.hip: film_record_block), into per-member slots the ensemble owns.

The reference for every record is Problem.film_integrals() -- k_film_partial + k_film_fold -- on the same state, held bit for
bit: film_record_block replays their summation order on one workgroup.  An LDS-tier member is bit for bit its solo run, so there
the solo problem's own set_integrals(1) series serves too; a workspace-tier member is bit for bit the same however its steps are
split into calls, so a second, freshly built ensemble stepped one step at a time gives the states to ask film_integrals() for.
Shapes: the smallest that reach each branch of the fold -- rows packed 64, 4, 2 and 1 to a wave, two and four virtual waves per
row, a thread's second pair, the half pair of an odd Ny, more rows than the 256 fold threads, in both tiers."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_ensemble import DIRICHLET, PL, assert_bitwise, bits, build, journal, mirror, quiet, records
from test_gpu_integrals import assert_same_series, flat

pytestmark = pytest.mark.gpu

PAIR = [journal(64, mc=1), journal(37, eps=0.5, edges=DIRICHLET)]      # 64 x 1 periodic, 37 x 1 Dirichlet


def asperity(nx, ny):
    """A 2-D member whose gap, and with V != 0 its state, vary along x AND y: the order of every sum matters."""
    return f"""
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: {2.5e-4 * nx}, Ly: {2.5e-4 * ny}, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 876.,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, max_it: 100000}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0.02, rho0: 877.7007}}
"""


def ensemble(cases, tier='auto'):
    from gapflow_amd import Ensemble
    ps = [build(t, s) for t, s in cases]
    return Ensemble(ps, tier=tier), ps


def now(p, sx=None, sy=None):
    """film_integrals() of p's state with the given sections (armed on p for the call only: an ensemble refuses an armed member)."""
    if sx is not None or sy is not None:
        p.set_integrals(10 ** 6, sx, sy)
    out = flat(p.film_integrals())
    p.clear_integrals()
    return out


def check_against_film_integrals(cases, n, tier='auto', tiers=None, sx=None, sy=None):
    """One step(n) at every = 1 against a second, freshly built ensemble stepped one step at a time with film_integrals() after
    each step: every record, its step and its time in every bit."""
    rec, _ = ensemble(cases, tier)
    if tiers is not None:
        assert rec.tiers == tiers
    rec.set_integrals(1, sx, sy)
    quiet(rec.step, n)
    series = rec.integrals
    twin, ps = ensemble(cases, tier)
    for k in range(n):
        quiet(twin.step, 1)
        for m, p in enumerate(ps):
            s = series[m]
            assert s.step.tolist() == list(range(1, n + 1)), f"member {m}"
            assert p.step == k + 1 and bits(s.time[k]) == bits(p.simtime), f"member {m}: time of step {k + 1}"
            got, want = flat(s, k), now(p, sx, sy)
            assert sorted(got) == sorted(want)
            assert np.isfinite(got['load']) and got['load'] != 0.0
            for q in want:
                assert bits(got[q]) == bits(want[q]), f"member {m}, step {k + 1}: {q} recorded {got[q]!r}, film_integrals() {want[q]!r}"
    return series


_SOLO = {}


def solo_series(text, n):
    """The same problem alone, set_integrals(1), n steps in one gpf_step: computed once, shared, left unchanged."""
    if (text, n) not in _SOLO:
        p = build(text)
        p.set_integrals(1)
        assert p.integrals_in_batch
        quiet(p._advance, n, honor_stop=False)
        _SOLO[(text, n)] = p.integrals
    return _SOLO[(text, n)]


def test_lds_tier_every_step_equals_the_solo_series(hiplib):
    """64 x 1 periodic and 37 x 1 Dirichlet, every = 1, step(9): each member's series is the solo problem's in every bit, step
    and time included; the members' own `integrals` stay None."""
    ens, ps = ensemble([(t, False) for t in PAIR])
    assert ens.integrals is None
    ens.set_integrals(1)
    assert [len(s.step) for s in ens.integrals] == [0, 0]
    quiet(ens.step, 9)
    for m, t in enumerate(PAIR):
        assert_same_series(ens.integrals[m], solo_series(t, 9), f"member {m}")
        assert type(ens.integrals[m]) is type(solo_series(t, 9)) and ps[m].integrals is None
        last = now(ps[m])
        for q, v in flat(ens.integrals[m], 8).items():
            assert bits(v) == bits(last[q]), f"member {m}: last record against film_integrals(): {q}"


def test_stride_across_calls_with_per_member_counts(hiplib):
    """every = 4; [5, 0] then [6, 7]: member 0 goes 0 -> 5 -> 11 and records steps 4 and 8 (one per call), member 1 goes
    0 -> 0 -> 7 and records step 4: the records of the solo every = 1 series at those steps."""
    ens, ps = ensemble([(t, False) for t in PAIR])
    ens.set_integrals(4)
    quiet(ens.step, [5, 0])
    assert [s.step.tolist() for s in ens.integrals] == [[4], []]
    have = C.c_int64(-1)
    assert hiplib.gpf_ensemble_integrals_read(ens._e, 1, None, 0, None, C.byref(have)) == 0 and have.value == 0
    quiet(ens.step, [6, 7])
    assert [p.step for p in ps] == [11, 7]
    assert [s.step.tolist() for s in ens.integrals] == [[4, 8], [4]]
    assert hiplib.gpf_ensemble_integrals_read(ens._e, 0, None, 0, None, C.byref(have)) == 0 and have.value == 1     # the last call's
    assert_same_series(solo_series(PAIR[0], 11), ens.integrals[0], 'member 0', pick=[3, 7])
    assert_same_series(solo_series(PAIR[1], 7), ens.integrals[1], 'member 1', pick=[3])


FOLD_LDS = {'300x1': [(journal(300), False)],                       # the row fold takes two rows per thread; 64 rows per wave
            '1x300': [(asperity(1, 300), False)],                   # 150 pairs over three virtual waves
            '20x13': [(asperity(20, 13), False)],                   # odd Ny: the half pair; 7 pairs, 8 rows per wave
            '9x30-slip+PL': [(asperity(9, 30), True),               # a slip-length field; 15 pairs, 4 rows per wave
                             (journal(33, eps=0.5, prop=PL, rho0=1.1853, edges=DIRICHLET, mc=1), False)]}


@pytest.mark.parametrize('name', list(FOLD_LDS))
def test_fold_branches_lds_tier(hiplib, name):
    check_against_film_integrals(FOLD_LDS[name], 3, tiers=['lds'] * len(FOLD_LDS[name]))


def test_explicit_sections_lds_tier(hiplib):
    """An interior row and column among the sections, the same for both members; a row named twice."""
    s = check_against_film_integrals([(asperity(20, 13), False), (asperity(9, 30), True)], 3, tiers=['lds', 'lds'], sx=[1, 5, 9, 5], sy=[2, 13])
    assert s[0].flow_x.shape == (3, 4) and s[1].flow_y.shape == (3, 2) and s[0].sections_x.tolist() == [1, 5, 9, 5]
    assert_bitwise(s[0].flow_x[:, 1], s[0].flow_x[:, 3], 'the row named twice')


FOLD_WORKSPACE = {'50x50': ([(asperity(50, 50), False)], 'auto'),
                  '3x600': ([(asperity(3, 600), False)], 'auto'),           # 300 pairs: a thread's second pair, four virtual waves
                  '520x1': ([(journal(520), False)], 'auto'),               # more rows than fold threads
                  '64x1-forced': ([(journal(64, mc=1), False)], 'workspace')}


@pytest.mark.parametrize('name', list(FOLD_WORKSPACE))
def test_workspace_tier(hiplib, name):
    cases, tier = FOLD_WORKSPACE[name]
    check_against_film_integrals(cases, 6, tier=tier, tiers=['workspace'] * len(cases))


def test_stop_and_rollback(hiplib):
    """run() with one member that stops at max_it = 7, one rolled back in its fourth step (an absurd dt, as
    test_gpu_integrals.test_rolled_back_step_leaves_no_record provokes it: a numerical rollback) and one that goes its 12 steps:
    each series ends or skips as the solo problem's does, and nobody's depends on the others."""
    from gapflow_amd import Ensemble
    texts = [journal(64, max_it=7, mc=1), journal(40, adaptive=0, dt='1e-10', max_it=12), journal(72, eps=0.5, max_it=12)]

    def spoil(p):
        p._lib.gpf_set_dt(p._h, 1.0)
        p.dt = 1.0

    alone = [build(t) for t in texts]
    for p in alone:
        p.set_integrals(1)
        quiet(p._advance, 3, honor_stop=False)
    spoil(alone[1])
    for p in alone:
        quiet(p.run)
    ps = [build(t) for t in texts]
    ens = Ensemble(ps)
    ens.set_integrals(1)
    quiet(ens.step, 3)
    spoil(ps[1])
    quiet(ens.run)
    assert [p.step for p in ps] == [p.step for p in alone] == [7, 3, 12] and ps[1]._stop
    for m, (p, s) in enumerate(zip(ps, alone)):
        assert_same_series(ens.integrals[m], s.integrals, f"member {m}")
    assert [len(s.step) for s in ens.integrals] == [7, 3, 12]


def test_recording_only_reads(hiplib):
    """The same ensemble (both tiers) with and without set_integrals(1): q, the scalars and the logs in every bit."""
    cases = [(journal(64, mc=1), False), (asperity(20, 13), False), (asperity(50, 50), False)]
    out = []
    for armed in (False, True):
        ens, ps = ensemble(cases)
        if armed:
            ens.set_integrals(1)
        logs = quiet(ens._advance, [9] * len(ps), honor_stop=False)
        out.append([(p.q.copy(), mirror(p), records(log)) for p, log in zip(ps, logs)])
    for m, ((q0, m0, l0), (q1, m1, l1)) in enumerate(zip(*out)):
        assert_bitwise(q1, q0, f"member {m}: q")
        assert m1[0] == m0[0] == 9
        assert_bitwise(m1[1:4], m0[1:4], f"member {m}: simtime, dt, residual")
        assert_bitwise(m1[4], m0[4], f"member {m}: residual_buffer")
        assert len(l0) == len(l1) == 9
        for a, b in zip(l1, l0):
            assert a[0] == b[0] and a[-2:] == b[-2:]
            assert_bitwise(a[1:-2], b[1:-2], f"member {m}: log")


def test_arguments_and_lifetime(hiplib):
    ens, ps = ensemble([(t, False) for t in PAIR])
    with pytest.raises(ValueError, match=r"member 1: .*sections_x\[1\] = 40"):
        ens.set_integrals(1, [1, 40])
    with pytest.raises(ValueError, match=r"member 0: .*sections_y\[0\] = 2"):
        ens.set_integrals(1, None, [2])
    with pytest.raises(ValueError, match='stride'):
        ens.set_integrals(0)
    assert ens.integrals is None
    # the library's own checks name the member and the section
    i32 = C.POINTER(C.c_int32)
    bad = np.array([1, 40], dtype=np.int32)
    assert hiplib.gpf_ensemble_integrals_set(ens._e, 1, 2, bad.ctypes.data_as(i32), 0, None) == -1
    assert b'member 1: x-section 1 at row 40' in hiplib.gpf_last_error()
    assert hiplib.gpf_ensemble_integrals_set(ens._e, 0, 0, None, 0, None) == -1 and b'every >= 1' in hiplib.gpf_last_error()
    have = C.c_int64(0)
    assert hiplib.gpf_ensemble_integrals_read(ens._e, 0, None, 0, None, C.byref(have)) == -5          # not armed
    assert [p.step for p in ps] == [0, 0]
    ens.set_integrals(2)
    quiet(ens.step, 4)
    assert [s.step.tolist() for s in ens.integrals] == [[2, 4], [2, 4]]
    ens.set_integrals(1)                            # a new series
    assert [len(s.step) for s in ens.integrals] == [0, 0]
    ens.clear_integrals()
    assert ens.integrals is None
    assert hiplib.gpf_ensemble_integrals_read(ens._e, 0, None, 0, None, C.byref(have)) == -5
    quiet(ens.step, 2)                              # disarmed: steps on, records nothing
    assert [p.step for p in ps] == [6, 6] and ens.integrals is None
    # a member armed on itself is refused as ever
    ps[0].set_integrals(1)
    with pytest.raises(NotImplementedError, match=r"member 0: .*integrals"):
        ens.step(1)
