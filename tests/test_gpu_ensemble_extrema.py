"""Field-extrema series of ensembles (gpf_ensemble_extrema_*, Ensemble.set_extrema / extrema): both one-workgroup kernels write the
record inside the batch, into per-member slots the ensemble owns.

Every comparison is bit for bit (values, cells, steps, times); no tolerance appears.  An LDS-tier member runs the body of
k_small_steps, so its reference is the same problem alone with Problem.set_extrema.  A workspace-tier member agrees with a solo
run only to rounding, but it is bit for bit the same however its steps are split into calls: a twin ensemble stepped `every`
steps per call gives the states, and Problem.field_extrema() -- k_extrema_partial + k_extrema_fold -- the record of each.
Shapes: the smallest that reach every branch of extrema_record_wide (csrc/extrema_kernels.hip) -- more interior cells than
threads (50 x 50), neither a multiple of 512 nor of 64 (37 x 11), fewer cells than threads (9 x 5: waves that hold no
candidate), Ny = 1 (64 x 1), and a field whose every extremum ties along iy (24 x 6, x-only gap)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_ensemble import assert_bitwise, bits, build, journal, mirror, quiet, records
from test_gpu_ensemble_integrals import PAIR, asperity, ensemble

pytestmark = pytest.mark.gpu

NAMES = ('p_max', 'p_min', 'rho_max', 'rho_min', 'h_min', 'u_max', 'v_max')


def assert_same_extrema(got, want, what, pick=None):
    """FieldExtrema `got` against `want` (its records `pick`, or all): steps, times, the seven values and the cells."""
    sel = slice(None) if pick is None else list(pick)
    assert type(got) is type(want) and got.index == want.index, what
    assert got.step.tolist() == want.step[sel].tolist(), f"{what}: steps {got.step.tolist()}"
    assert_bitwise(got.time, want.time[sel], f"{what}: time")
    for name in NAMES:
        assert_bitwise(getattr(got, name), getattr(want, name)[sel], f"{what}: {name}")
    assert got.cells.dtype == np.int32 and np.array_equal(got.cells, want.cells[sel]), f"{what}: cells"


_SOLO = {}


def solo_series(text, n):
    """The same problem alone, set_extrema(1), n steps in one gpf_step (k_small_steps): computed once, shared, left unchanged."""
    if (text, n) not in _SOLO:
        p = build(text)
        p.set_extrema(1)
        quiet(p._advance, n, honor_stop=False)
        assert p.step == n
        _SOLO[(text, n)] = p.extrema
    return _SOLO[(text, n)]


def test_lds_tier_every_step_equals_the_solo_series(hiplib):
    ens, ps = ensemble([(t, False) for t in PAIR])
    assert ens.tiers == ['lds', 'lds'] and ens.extrema is None
    ens.set_extrema(1)
    assert [len(s.step) for s in ens.extrema] == [0, 0]
    quiet(ens.step, 40)
    for m, t in enumerate(PAIR):
        want = solo_series(t, 40)
        assert want.step.tolist() == list(range(1, 41)) and np.ptp(want.p_max) > 0
        assert_same_extrema(ens.extrema[m], want, f"member {m}")
        assert ps[m].extrema is None
        now = ps[m].field_extrema()
        for k, name in enumerate(NAMES):
            assert bits(ens.extrema[m]._asdict()[name][-1]) == bits(now[name]), f"member {m}: last record against field_extrema(): {name}"
            assert tuple(ens.extrema[m].cells[-1, k]) == now[name + '_cell']


def test_stride_and_uneven_calls(hiplib):
    """every = 3; [5, 0], [4, 7], [3, 2]: member 0 goes 0 -> 5 -> 9 -> 12, member 1 goes 0 -> 0 -> 7 -> 9; the recorded steps are the
    multiples of 3 each passed, the records those of the solo every = 1 series at these steps; 0 steps leave a series untouched."""
    ens, ps = ensemble([(t, False) for t in PAIR])
    ens.set_extrema(3)
    quiet(ens.step, [5, 0])
    assert [s.step.tolist() for s in ens.extrema] == [[3], []]
    have = C.c_int64(-1)
    assert hiplib.gpf_ensemble_extrema_read(ens._e, 1, None, None, 0, None, C.byref(have)) == 0 and have.value == 0
    quiet(ens.step, [4, 7])
    assert [s.step.tolist() for s in ens.extrema] == [[3, 6, 9], [3, 6]]
    assert hiplib.gpf_ensemble_extrema_read(ens._e, 0, None, None, 0, None, C.byref(have)) == 0 and have.value == 2     # the last call's
    kept = ens.extrema[1]
    quiet(ens.step, [3, 0])
    assert_same_extrema(ens.extrema[1], kept, 'member 1 after a call with 0 steps')
    quiet(ens.step, [0, 2])
    assert [p.step for p in ps] == [12, 9]
    assert_same_extrema(ens.extrema[0], solo_series(PAIR[0], 12), 'member 0', pick=[2, 5, 8, 11])
    assert_same_extrema(ens.extrema[1], solo_series(PAIR[1], 12), 'member 1', pick=[2, 5, 8])


def check_against_field_extrema(cases, n, every, tier='auto'):
    """One step(n) at the stride against a second, freshly built ensemble stepped `every` steps per call with field_extrema()
    after each call: every record, its cells, its step and its time."""
    rec, _ = ensemble(cases, tier)
    assert rec.tiers == ['workspace'] * len(cases)
    rec.set_extrema(every)
    quiet(rec.step, n)
    series = rec.extrema
    twin, ps = ensemble(cases, tier)
    for k in range(n // every):
        quiet(twin.step, every)
        for m, p in enumerate(ps):
            s = series[m]
            assert s.step.tolist() == list(range(every, n + 1, every)), f"member {m}"
            assert p.step == (k + 1) * every and bits(s.time[k]) == bits(p.simtime), f"member {m}: time of step {p.step}"
            now = p.field_extrema()
            for j, name in enumerate(NAMES):
                got = getattr(s, name)[k]
                assert np.isfinite(got)
                assert bits(got) == bits(now[name]), f"member {m}, step {p.step}: {name} recorded {got!r}, field_extrema() {now[name]!r}"
                assert tuple(int(v) for v in s.cells[k, j]) == now[name + '_cell'], f"member {m}, step {p.step}: cell of {name}"
    return series, ps


WORKSPACE = {'50x50': ([(asperity(50, 50), False)], 'auto'),            # five interior cells per thread
             '64x1-forced': ([(journal(64, mc=1), False)], 'workspace'),       # Ny = 1: the cursor's width is 1
             '37x11-forced': ([(asperity(37, 11), False)], 'workspace'),       # 407 cells: no multiple of 64, a ragged last wave
             '9x5-forced': ([(asperity(9, 5), True)], 'workspace')}            # 45 cells: seven waves hold no candidate; slip-length field


@pytest.mark.parametrize('every', [1, 3])
@pytest.mark.parametrize('name', list(WORKSPACE))
def test_workspace_tier(hiplib, name, every):
    cases, tier = WORKSPACE[name]
    series, _ = check_against_field_extrema(cases, 12, every, tier)
    assert np.ptp(series[0].p_max) > 0 or np.ptp(series[0].u_max) > 0          # the state moves


def test_ties_go_to_the_smallest_ix_then_iy(hiplib):
    """24 x 6, the gap a function of x alone and V = 0: every column is the same in every bit, so every extremum is attained at
    six cells that the walk hands to different threads and waves; the record names the one with the smallest iy."""
    series, ps = check_against_field_extrema([(journal(24, ny=6, mc=1), False)], 12, 1, 'workspace')
    s, q = series[0], ps[0].q
    assert all(np.array_equal(bits(q[:, :, 1]), bits(q[:, :, j])) for j in range(2, 7)), 'the columns differ'
    rho = q[0, 1:-1, 1:-1]
    ix, iy = (int(v) for v in s.cells[-1, s.index['p_max']])
    # p is a function of the density alone: the maximum of p is attained at every cell that holds this density
    ties = np.argwhere(bits(rho) == bits(rho[ix - 1, iy - 1])) + 1
    assert len(ties) > 1 and (ix, iy) == tuple(ties[0]) and iy == 1, ties
    for name in ('rho_max', 'rho_min'):
        best = rho.max() if name == 'rho_max' else rho.min()
        first = np.argwhere(rho == best)[0] + 1
        assert len(np.argwhere(rho == best)) > 1 and tuple(s.cells[-1, s.index[name]]) == tuple(first), name
    assert (s.cells[:, :, 1] == 1).all()


def test_stop_and_rollback(hiplib):
    """run() with one member that stops at max_it = 7, one rolled back in its fourth step (an absurd dt: a numerical rollback that
    the step handles) and one that goes its 12 steps: records exist exactly for the committed steps, as in the solo runs."""
    from gapflow_amd import Ensemble
    texts = [journal(64, max_it=7, mc=1), journal(40, adaptive=0, dt='1e-10', max_it=12), journal(72, eps=0.5, max_it=12)]

    def spoil(p):
        p._lib.gpf_set_dt(p._h, 1.0)
        p.dt = 1.0

    alone = [build(t) for t in texts]
    for p in alone:
        p.set_extrema(1)
        quiet(p._advance, 3, honor_stop=False)
    spoil(alone[1])
    for p in alone:
        quiet(p.run)
    ps = [build(t) for t in texts]
    ens = Ensemble(ps)
    ens.set_extrema(1)
    quiet(ens.step, 3)
    spoil(ps[1])
    quiet(ens.run)
    assert [p.step for p in ps] == [p.step for p in alone] == [7, 3, 12] and ps[1]._stop
    for m, (p, s) in enumerate(zip(ps, alone)):
        assert_same_extrema(ens.extrema[m], s.extrema, f"member {m}")
    assert [s.step.tolist() for s in ens.extrema] == [list(range(1, 8)), [1, 2, 3], list(range(1, 13))]
    # the same in the workspace tier, against the members' own states: a twin stopped by hand where these stopped
    ws = [build(t) for t in texts]
    ens = Ensemble(ws, tier='workspace')
    ens.set_extrema(2)
    quiet(ens.step, 3)
    spoil(ws[1])
    quiet(ens.run)
    assert [p.step for p in ws] == [7, 3, 12]
    assert [s.step.tolist() for s in ens.extrema] == [[2, 4, 6], [2], [2, 4, 6, 8, 10, 12]]
    last = ws[2].field_extrema()
    assert all(bits(getattr(ens.extrema[2], name)[-1]) == bits(last[name]) for name in NAMES)


@pytest.mark.parametrize('tier', ['auto', 'workspace'])
def test_recording_only_reads(hiplib, tier):
    """The same ensemble with all three series armed and with none: q, the scalars and the logs of 30 steps in every bit."""
    cases = [(journal(64, mc=1), False), (asperity(20, 13), True)] + ([(asperity(50, 50), False)] if tier == 'auto' else [])
    out = []
    for armed in (False, True):
        ens, ps = ensemble(cases, tier)
        if armed:
            ens.set_integrals(2)
            ens.set_extrema(1)
            ens.set_probes([[0, 0], [1, 1], [3, 1]])
        logs = quiet(ens._advance, [30] * len(ps), honor_stop=False)
        if armed:
            assert [len(s.step) for s in ens.integrals] == [15] * len(ps)
            assert [len(s.step) for s in ens.extrema] == [len(s.step) for s in ens.probes] == [30] * len(ps)
        out.append([(p.q.copy(), mirror(p), records(log)) for p, log in zip(ps, logs)])
    for m, ((q0, m0, l0), (q1, m1, l1)) in enumerate(zip(*out)):
        assert_bitwise(q1, q0, f"member {m}: q")
        assert m1[0] == m0[0] == 30
        assert_bitwise(m1[1:4], m0[1:4], f"member {m}: simtime, dt, residual")
        assert_bitwise(m1[4], m0[4], f"member {m}: residual_buffer")
        assert len(l0) == len(l1) == 30
        for a, b in zip(l1, l0):
            assert a[0] == b[0] and a[-2:] == b[-2:]
            assert_bitwise(a[1:-2], b[1:-2], f"member {m}: log")


def test_arguments_and_lifetime(hiplib):
    ens, ps = ensemble([(t, False) for t in PAIR])
    with pytest.raises(ValueError, match='stride'):
        ens.set_extrema(0)
    assert ens.extrema is None
    assert hiplib.gpf_ensemble_extrema_set(ens._e, 0) == -1 and b'every >= 1' in hiplib.gpf_last_error()
    have = C.c_int64(0)
    assert hiplib.gpf_ensemble_extrema_read(ens._e, 0, None, None, 0, None, C.byref(have)) == -5         # read before set
    assert hiplib.gpf_ensemble_extrema_read(ens._e, 2, None, None, 0, None, C.byref(have)) == -1 and b'member 2' in hiplib.gpf_last_error()
    assert [p.step for p in ps] == [0, 0]
    ens.set_extrema(2)
    quiet(ens.step, 4)
    assert [s.step.tolist() for s in ens.extrema] == [[2, 4], [2, 4]]
    ens.set_extrema(1)                              # set twice: new series
    assert [len(s.step) for s in ens.extrema] == [0, 0]
    quiet(ens.step, 1)
    assert [s.step.tolist() for s in ens.extrema] == [[5], [5]]
    ens.clear_extrema()
    assert ens.extrema is None
    assert hiplib.gpf_ensemble_extrema_read(ens._e, 0, None, None, 0, None, C.byref(have)) == -5
    quiet(ens.step, 2)                              # clear, then step: steps on, records nothing
    assert [p.step for p in ps] == [7, 7] and ens.extrema is None
    ens.clear_extrema()                             # not armed: nothing to do
    # a member armed on itself is refused as ever, in the existing words
    ps[0].set_extrema(1)
    with pytest.raises(NotImplementedError, match=r"member 0: extrema are armed on it \(their records need per-member slots\)"):
        ens.step(1)
    armed = build(PAIR[0])
    armed.set_extrema(1)
    from gapflow_amd import Ensemble
    with pytest.raises(NotImplementedError, match=r"member 1: extrema are armed on it \(their records need per-member slots\): clear_extrema\(\), or run it alone"):
        Ensemble([build(PAIR[1]), armed])


def test_run_writes_extrema_npz(hiplib, tmp_path):
    """A non-silent member's series goes to extrema.npz when its run ends: the arrays a solo run writes."""
    from gapflow_amd import Ensemble
    opts = [f"output: {tmp_path / name}, write_freq: 100, use_tstamp: False, silent: False" for name in ('ens', 'solo')]
    p, alone = build(journal(64, max_it=6, mc=1, options=opts[0])), build(journal(64, max_it=6, mc=1, options=opts[1]))
    alone.set_extrema(2)
    quiet(alone.run)
    ens = Ensemble([p])
    ens.set_extrema(2)
    quiet(ens.run)
    got, want = np.load(tmp_path / 'ens' / 'extrema.npz'), np.load(tmp_path / 'solo' / 'extrema.npz')
    assert sorted(got.files) == sorted(want.files) and got['step'].tolist() == [2, 4, 6]
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k
