"""Film integrals of a problem alone on the one-workgroup kernel: k_small_steps writes the record inside the batch
(csrc/integral_kernels.hip: film_record_block) instead of having the batch cut at every recorded step.

Reference: Problem.film_integrals() -- k_film_partial + k_film_fold -- on the same state, bit for bit; the series and the runs
of tests/test_gpu_integrals.py (case 'small-1d': the 100 x 1 journal bearing) are shared, not recomputed."""
import numpy as np
import pytest

import test_gpu_integrals as tgi
from test_gpu_probes import JOURNAL_1D, assert_bitwise, bits, build

pytestmark = pytest.mark.gpu


def test_which_path_a_problem_takes(hiplib):
    small = build(JOURNAL_1D)
    assert small.integrals_in_batch is False        # not armed
    small.set_integrals(1)
    assert small.integrals_in_batch is True
    small.clear_integrals()
    assert small.integrals_in_batch is False
    wide = build(tgi.PIEZO_WIDE)                    # 300 columns: off the small kernel
    wide.set_integrals(1)
    assert wide.integrals_in_batch is False


def test_every_step_of_one_batch_equals_film_integrals(hiplib):
    """every = 1 over 50 steps in ONE launch against film_integrals() of the twin after each of its 50 update() calls."""
    r = tgi.case_runs('small-1d')
    s = r['series']
    assert s.step.tolist() == list(range(1, 51))
    assert_bitwise(s.time, r['twin_times'], 'time')
    for k in range(50):
        got, now = tgi.flat(s, k), r['now'][k]
        for q in now:
            assert bits(got[q]) == bits(now[q]), f"step {k + 1}: {q} recorded {got[q]!r}, film_integrals() {now[q]!r}"


def test_beside_a_series_that_cuts_the_batch(hiplib):
    """Weighted integrals at stride 7 still cut the batch; film integrals at stride 3 ride inside its pieces (7, 7, ..., 1 steps):
    the cursor finds each piece's first record and slot.  Both series are bitwise those of separate runs."""
    w = np.linspace(0., 1., 100)[:, None] ** 2
    both, film, weighted = build(JOURNAL_1D), build(JOURNAL_1D), build(JOURNAL_1D)
    both.set_integrals(3)
    both.set_weighted_integrals(w, 7)
    film.set_integrals(3)
    weighted.set_weighted_integrals(w, 7)
    for p in (both, film, weighted):
        p._advance(50, honor_stop=False)
    assert both.integrals_in_batch and both.integrals.step.tolist() == list(range(3, 51, 3))
    tgi.assert_same_series(both.integrals, film.integrals, 'film integrals beside weighted ones')
    tgi.assert_same_series(tgi.case_runs('small-1d')['series'], both.integrals, 'against every = 1', pick=list(range(2, 50, 3)))
    a, b = both.weighted_integrals, weighted.weighted_integrals
    assert a.step.tolist() == b.step.tolist() == list(range(7, 51, 7))
    for name in a._fields:
        if name not in ('step', 'names'):
            assert_bitwise(getattr(a, name), getattr(b, name), f"weighted integrals beside film ones: {name}")
