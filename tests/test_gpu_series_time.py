"""The seven gpf_*_time diagnostics (probes, film integrals, weighted integrals, regions, lines, extrema, statistics), held to the
one rule include/gapflow_hip.h states for them: a call advances the state exactly as gpf_step does, records the series it times
(mode 1) exactly as gpf_step does, puts every other series aside and leaves none of their records, restarts an armed statistics
window unless it recorded into it, and leaves every series armed as it was.

Two identical problems, A and B, with all seven series armed at unequal strides, advanced 5 steps; then A takes 12 steps through
gpf_<series>_time and B through gpf_step, and both take 6 more through gpf_step.  Everything is compared bit for bit between the
two, on both step paths: JOURNAL_1D (100 x 1, k_small_steps) and journal_2d(37, 71) (2847 ghosted cells, k_step2).  After the raw
gpf_*_time call the Python mirror of the step count is stale, so from there on both problems are driven through ctypes.

Messages that begin with (a) or (b) name the two parts of the rule that are the same for all seven calls by the shared frame
(csrc/api_series.inc: series_time) alone: (a) gpf_probes_time restarts the window too, (b) no other series keeps the previous
call's records."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_extrema import bits, build, journal_2d
from test_gpu_probes import JOURNAL_1D

pytestmark = pytest.mark.gpu

SERIES = ('probes', 'integrals', 'weighted', 'regions', 'lines', 'extrema', 'stats')
STRIDED = SERIES[1:6]
GRIDS = {'small-1d': JOURNAL_1D, 'step2-37x71': journal_2d(37, 71)}
WARM, TIMED, AFTER = 5, 12, 6
CAP = 32                # records a read has room for: more than any call here leaves
I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)


def armed(text):
    """A problem with all seven series armed at unequal strides, WARM steps in."""
    p = build(text)
    nx, ny = p.grid['Nx'], p.grid['Ny']
    p.set_probes([(1, 1), (nx // 2, (ny + 1) // 2), (nx, ny)])
    p.set_integrals(2)
    p.set_weighted_integrals(np.ones((nx, ny)), 3)
    p.set_regions([{'field': 'rho'}], 4)            # no bounds, no box: the whole interior
    p.set_lines([{'along': 'x'}], 3)                # the centre line
    p.set_extrema(2)
    p.set_statistics(2)
    p._advance(WARM, False)
    return p


def ok(p, code):
    assert code == 0, p._lib.gpf_last_error()


def step(p, n):
    ok(p, p._lib.gpf_step(p._h, n, 0, None, 0, None))


def timed(p, series, n, mode):
    ms = C.c_double(-1.)
    ok(p, getattr(p._lib, f'gpf_{series}_time')(p._h, n, mode, C.byref(ms)))
    return ms.value


def step_count(p):
    from gapflow_amd import _lib
    sc = _lib.GpfScalars()
    ok(p, p._lib.gpf_scalars(p._h, C.byref(sc)))
    return int(sc.step)


def state(p):
    from gapflow_amd import _lib
    q = np.zeros((3,) + tuple(p._shape))
    ok(p, p._lib.gpf_download(p._h, _lib.FIELD_Q, _lib.as_dp(q), q.size))
    return q


def records(p, series):
    """(number of records, their step counts, their values as one tuple of zero-padded arrays) of the last stepping call."""
    from gapflow_amd import _lib
    lib, h = p._lib, p._h
    n, steps = C.c_int64(-1), np.zeros(CAP, dtype=np.int64)
    vals, ints = np.zeros((CAP, 1024)), np.zeros((CAP, 16), dtype=np.int64)
    sp, np_ = steps.ctypes.data_as(I64P), C.byref(n)
    if series == 'probes':
        first = C.c_int64(0)
        ok(p, lib.gpf_probes_read(h, _lib.as_dp(vals), CAP, C.byref(first), np_))
        steps[:n.value] = first.value + np.arange(n.value)
    elif series == 'regions':
        ok(p, lib.gpf_regions_read(h, _lib.as_dp(vals), ints.ctypes.data_as(I64P), CAP, sp, np_))
    elif series == 'extrema':
        cells = np.zeros((CAP, 14), dtype=np.int32)
        ok(p, lib.gpf_extrema_read(h, _lib.as_dp(vals), cells.ctypes.data_as(I32P), CAP, sp, np_))
        ints[:, :14] = cells
    else:
        ok(p, getattr(lib, f'gpf_{series}_read')(h, _lib.as_dp(vals), CAP, sp, np_))
    assert 0 <= n.value <= CAP
    return n.value, steps, (vals, ints)


def window(p):
    """(count, first_step, last_step) of the statistics window"""
    c, f, l = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok(p, p._lib.gpf_stats_info(p._h, C.byref(c), C.byref(f), C.byref(l), None, None))
    return c.value, f.value, l.value


def stats_planes(p):
    """mean and m2 of the four fields"""
    from gapflow_amd import _lib
    out = np.zeros((4, 2) + tuple(p._shape))
    for f in range(4):
        for k in range(2):
            ok(p, p._lib.gpf_stats_read(p._h, f, k, _lib.as_dp(out[f, k]), out[f, k].size))
    return out


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def same_records(ra, rb):
    return ra[0] == rb[0] and (ra[1] == rb[1]).all() and same_bits(ra[2][0], rb[2][0]) and (ra[2][1] == rb[2][1]).all()


class Findings(list):
    """Every broken expectation of a case, not only the first"""
    def expect(self, cond, what):
        if not cond:
            self.append(what)

    def settle(self):
        assert not self, f"{len(self)} expectation(s) broken:\n  " + "\n  ".join(self)


def expect_same_run_after(f, a, b, what):
    """AFTER more steps through gpf_step on both: every series records the same -- the strides were put back"""
    step(a, AFTER)
    step(b, AFTER)
    f.expect(step_count(a) == step_count(b) == WARM + TIMED + AFTER, f"{what}: step counts {step_count(a)} and {step_count(b)}")
    f.expect(same_bits(state(a), state(b)), f"{what}: the states differ")
    for s in SERIES[:6]:
        ra, rb = records(a, s), records(b, s)
        f.expect(rb[0] > 0, f"{what}: the gpf_step twin recorded no {s}")
        f.expect(same_records(ra, rb), f"{what}: {s} differ ({ra[0]} records at {ra[1][:ra[0]].tolist()}, the twin's {rb[0]} at {rb[1][:rb[0]].tolist()})")


@pytest.mark.parametrize('series', SERIES)
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_mode_1_records_its_series_as_gpf_step_does_and_no_other(hiplib, grid, series):
    a, b = armed(GRIDS[grid]), armed(GRIDS[grid])
    f = Findings()
    ms = timed(a, series, TIMED, 1)
    step(b, TIMED)
    f.expect(np.isfinite(ms) and ms > 0, f"ms = {ms}")
    f.expect(step_count(a) == step_count(b) == WARM + TIMED, f"step counts {step_count(a)} and {step_count(b)}")
    f.expect(same_bits(state(a), state(b)), "the states differ after the timed steps")
    for s in SERIES[:6]:
        ra = records(a, s)
        if s == series:
            rb = records(b, s)
            f.expect(rb[0] > 0, f"the gpf_step twin recorded no {s}")
            f.expect(same_records(ra, rb), f"the timed {s} differ from gpf_step's ({ra[0]} records, the twin's {rb[0]})")
        else:
            f.expect(ra[0] == 0, f"(b) {s} report {ra[0]} records after gpf_{series}_time")
    if series == 'stats':
        f.expect(window(a) == window(b), f"the window did not continue: {window(a)}, gpf_step's {window(b)}")
    else:
        f.expect(window(a)[0] == 0, f"{'(a) ' if series == 'probes' else ''}the statistics window was not restarted: {window(a)}")
    expect_same_run_after(f, a, b, "after mode 1")
    if series == 'stats':
        f.expect(window(a) == window(b), f"the window after the next call: {window(a)}, gpf_step's {window(b)}")
        f.expect(same_bits(stats_planes(a), stats_planes(b)), "mean / m2 planes differ")
    else:
        count, first, _ = window(a)
        f.expect(count == AFTER // 2 and first > WARM + TIMED,
                 f"{'(a) ' if series == 'probes' else ''}the window after the next call: {window(a)}, {AFTER // 2} records from step {WARM + TIMED + 1} on expected")
    f.settle()


@pytest.mark.parametrize('series', SERIES)
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_mode_0_steps_as_gpf_step_does_and_records_nothing(hiplib, grid, series):
    a, b = armed(GRIDS[grid]), armed(GRIDS[grid])
    f = Findings()
    ms = timed(a, series, TIMED, 0)
    step(b, TIMED)
    f.expect(np.isfinite(ms) and ms > 0, f"ms = {ms}")
    f.expect(step_count(a) == step_count(b) == WARM + TIMED, f"step counts {step_count(a)} and {step_count(b)}")
    f.expect(same_bits(state(a), state(b)), "the states differ after the timed steps")
    if series != 'stats':
        f.expect(records(a, series)[0] == 0, f"{series} report {records(a, series)[0]} records after mode 0")
    else:
        f.expect(window(a)[0] == 0, f"the statistics window was not restarted: {window(a)}")
    expect_same_run_after(f, a, b, "after mode 0")
    f.settle()


def test_probes_mode_2_leaves_the_state_of_plain_steps(hiplib):
    a, b = armed(GRIDS['step2-37x71']), armed(GRIDS['step2-37x71'])
    ms = timed(a, 'probes', TIMED, 2)
    step(b, TIMED)
    assert np.isfinite(ms) and ms > 0
    assert step_count(a) == step_count(b) == WARM + TIMED
    assert same_bits(state(a), state(b))


def test_stats_mode_2_takes_no_step_and_restarts_the_window(hiplib):
    a = armed(GRIDS['step2-37x71'])
    before = state(a)
    assert window(a)[0] == WARM // 2
    ms = timed(a, 'stats', TIMED, 2)
    assert np.isfinite(ms) and ms > 0
    assert step_count(a) == WARM and same_bits(state(a), before)
    assert window(a)[0] == 0
