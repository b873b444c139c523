"""The series' host side (gapflow_amd/series.py): the one recorder `_Series` against a brute-force filter of the committed steps,
its mismatch branch (the sentence every series raised before it), the lifecycle table against Problem and Ensemble's refusals,
and `_keep_own_options` against the ten `_keep_*` functions applied one after the other.  No GPU, no device call, no library."""
import inspect
import io
import types

import numpy as np
import pytest

ALL_KEYS = """
options: {silent: True, checkpoint_freq: 12, probes: [[0, 1], [50, 3]], probes_pressure: False, integrals: 2,
          integrals_sections_x: [1, 50, 100], integrals_sections_y: [2], extrema: 1, elastic_series: 3, weighted_integrals: 3,
          weights: [{box: [1, 50, 1, 3], name: pad}], statistics: 2, statistics_fields: [rho, p], statistics_after: 4, regions: 5,
          region_list: [{field: rho, below: 850.0, name: cavitated}], lines: 4, line_list: [{along: x}, {along: y, at: [1, 32], name: band}],
          init_from: coarse/checkpoint.gpf}
grid: {Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}
"""
TWO_BUFFERS = [((3, 9), np.float64), ((3, 5), np.int64)]            # the regions' sums and ints
LABELS = ['integrals', 'Ensemble integrals: member 3']


def entries_of(before, ran):
    return [types.SimpleNamespace(step=s, simtime=0.5 * s) for s in range(before + 1, before + ran + 1)]


def multiples(before, ran, every):
    return [s for s in range(before + 1, before + ran + 1) if s % every == 0]


def library(before, ran, every, short=0, wrong=None):
    """A `read` that fills what the library would: record i of every buffer holds its step number; `short` records are held back,
    record `wrong` names the step after its own."""
    calls = []

    def read(buffers, n, steps_ptr, have_ref):
        calls.append(n)
        want = multiples(before, ran, every)
        assert n == len(want)                       # the capacity asked for is the count of the multiples
        for i, s in enumerate(want[:len(want) - short]):
            steps_ptr[i] = s + 1 if i == wrong else s
            for b in buffers:
                b[i] = s
        have_ref[0] = len(want) - short
    read.calls = calls
    return read


@pytest.mark.parametrize('every', [1, 3, 7])
@pytest.mark.parametrize('before', [0, 5, 6])
def test_collect_keeps_the_multiples_of_the_stride(every, before):
    from gapflow_amd.series import _Series
    for ran in range(1, 14):
        s = _Series('regions', every)
        want = multiples(before, ran, every)
        s.collect(library(before, ran, every), entries_of(before, ran), before, TWO_BUFFERS)
        assert s.steps == want and s.times == [0.5 * k for k in want]
        assert s.step_array().dtype == np.int64 and s.step_array().tolist() == want
        assert s.time_array().dtype == np.float64 and s.time_array().tolist() == [0.5 * k for k in want]
        sums, ints = s.stacked(0, (3, 9)), s.stacked(1, (3, 5), np.int64)
        assert sums.dtype == np.float64 and sums.shape == (len(want), 3, 9) and ints.dtype == np.int64 and ints.shape == (len(want), 3, 5)
        assert all((sums[i] == k).all() and (ints[i] == k).all() for i, k in enumerate(want))
        # the next call goes on where this one ended, and its block lands behind the first
        s.collect(library(before + ran, 4, every), entries_of(before + ran, 4), before + ran, TWO_BUFFERS)
        both = multiples(before, ran + 4, every)
        assert s.steps == both and len(s.blocks) == 2 and s.stacked(1, (3, 5), np.int64)[:, 0, 0].tolist() == both


def test_two_buffer_blocks_keep_their_dtypes():
    from gapflow_amd.series import _Series
    s = _Series('extrema', 1)
    s.collect(library(0, 3, 1), entries_of(0, 3), 0, [((7,), np.float64), ((7, 2), np.int32)])
    assert [b.dtype for b in s.blocks[0]] == [np.float64, np.int32]
    assert s.stacked(1, (7, 2), np.int32).dtype == np.int32 and s.stacked(1, (7, 2), np.int32).shape == (3, 7, 2)


def test_an_empty_series_stacks_to_the_empty_shape():
    from gapflow_amd.series import _Series
    s = _Series('extrema', 2)
    for k, shape, dtype in ((0, (7,), np.float64), (1, (7, 2), np.int32), (1, (3, 5), np.int64), (0, (), np.float64)):
        a = s.stacked(k, shape, dtype)
        assert a.shape == (0,) + shape and a.dtype == dtype
    assert s.step_array().shape == (0,) and s.step_array().dtype == np.int64 and s.time_array().dtype == np.float64
    read = library(0, 0, 2)
    s.collect(read, [], 0, TWO_BUFFERS)             # a call that committed nothing reads nothing
    assert read.calls == [] and s.blocks == []
    s.collect(library(0, 1, 2), entries_of(0, 1), 0, TWO_BUFFERS)       # one that committed no multiple leaves an empty block
    assert s.steps == [] and s.stacked(1, (3, 5), np.int64).shape == (0, 3, 5)
    s.reset()
    assert (s.steps, s.times, s.blocks) == ([], [], [])


@pytest.mark.parametrize('label', LABELS)
def test_a_record_too_few_raises_the_sentence_and_appends_nothing(label):
    from gapflow_amd._lib import GapflowHipError
    from gapflow_amd.series import _Series
    s = _Series(label, 2)
    s.collect(library(0, 4, 2), entries_of(0, 4), 0, TWO_BUFFERS)
    with pytest.raises(GapflowHipError) as err:
        s.collect(library(4, 6, 2, short=1), entries_of(4, 6), 4, TWO_BUFFERS)
    assert str(err.value) == f"{label}: 2 records of steps [6, 8, 0] for the committed steps 5..10 at stride 2"
    assert s.steps == [2, 4] and s.times == [1.0, 2.0] and len(s.blocks) == 1


@pytest.mark.parametrize('label', LABELS)
def test_a_wrong_step_raises_the_sentence_and_appends_nothing(label):
    from gapflow_amd._lib import GapflowHipError
    from gapflow_amd.series import _Series
    s = _Series(label, 3)
    with pytest.raises(GapflowHipError) as err:
        s.collect(library(5, 7, 3, wrong=1), entries_of(5, 7), 5, TWO_BUFFERS)
    assert str(err.value) == f"{label}: 3 records of steps [6, 10, 12] for the committed steps 6..12 at stride 3"
    assert (s.steps, s.times, s.blocks) == ([], [], [])


def test_the_probes_record_every_step_and_keep_their_own_sentence():
    from gapflow_amd._lib import GapflowHipError
    from gapflow_amd.series import _Series

    def library_of(first, have):
        def read(out, n, first_ref, have_ref):
            out[:have] = np.arange(first, first + have).reshape(-1, 1, 1)
            first_ref[0], have_ref[0] = first, have
        return read
    s = _Series('probes')
    s.collect_every_step(library_of(6, 3), entries_of(5, 3), (2, 4))
    assert s.steps == [6, 7, 8] and s.times == [3.0, 3.5, 4.0] and s.stacked(0, (2, 4))[:, 1, 3].tolist() == [6.0, 7.0, 8.0]
    for first, have, said in ((9, 2, "probes: 2 records from step 9 for 3 committed steps from step 9"),
                              (10, 3, "probes: 3 records from step 10 for 3 committed steps from step 9")):
        with pytest.raises(GapflowHipError) as err:
            s.collect_every_step(library_of(first, have), entries_of(8, 3), (2, 4))
        assert str(err.value) == said
    assert s.steps == [6, 7, 8] and len(s.blocks) == 1
    assert _Series('probes').stacked(0, (2, 4)).shape == (0, 2, 4)


def test_the_table_names_what_problem_has():
    from gapflow_amd import Problem
    from gapflow_amd.series import SERIES
    arming = inspect.getsource(Problem.__init__)
    assert [r.marker for r in SERIES] == ['_probe_cells', '_integral_every', '_weighted_every', '_regions_every', '_lines_every',
                                          '_extrema_every', '_elastic_series_every', '_stats_every']
    for row in SERIES:
        assert f"self.{row.marker} = None" in arming, f"Problem.__init__ does not start with {row.marker} off"
        assert callable(getattr(Problem, row.write)) and callable(getattr(Problem, row.clear))
        assert row.collect is None or callable(getattr(Problem, row.collect))
        assert (row.collect is None) == (row.recorder is None)
    assert [r.marker for r in SERIES if not r.fused] == ['_elastic_series_every', '_stats_every']


# Ensemble's refusals as they read before the table, in their order of precedence
REFUSALS = [('_integral_every', "film integrals are armed on it (they cut the batch per member): clear_integrals(), or run it alone"),
            ('_weighted_every', "weighted integrals are armed on it (they cut the batch per member): clear_weighted_integrals(), or run it alone"),
            ('_stats_every', "statistics are armed on it (they cut the batch per member): clear_statistics(), or run it alone"),
            ('_regions_every', "regions are armed on it (they cut the batch per member): clear_regions(), or run it alone"),
            ('_lines_every', "lines are armed on it (they cut the batch per member): clear_lines(), or run it alone"),
            ('_probe_cells', "probes are armed on it (their records need per-member slots): clear_probes(), or run it alone"),
            ('_extrema_every', "extrema are armed on it (their records need per-member slots): clear_extrema(), or run it alone")]


def test_refusal_says_the_seven_sentences_in_their_order(monkeypatch):
    from gapflow_amd import Problem
    from gapflow_amd.ensemble import _refusal
    monkeypatch.delenv('GPF_SMALL_GRID', raising=False)
    p = Problem.__new__(Problem)
    p._gp_models, p.has_gp_model, p._elastic = {}, False, None
    p._cfg = types.SimpleNamespace(thinning=0, device=0)
    p.topo = types.SimpleNamespace(elastic=False)
    p._shape, p.grid = (102, 3), {'Nx': 100, 'Ny': 1}
    assert _refusal(p) is None                      # an object that has none of the markers is a member
    for marker, _ in REFUSALS:
        setattr(p, marker, 1)
    p._elastic_series_every = 1                     # (never asked: an elastic gap is refused before the series are looked at)
    for marker, sentence in REFUSALS:               # with all that follow still armed, the first in the order is named
        assert _refusal(p) == (NotImplementedError, sentence)
        setattr(p, marker, None)
    assert _refusal(p) is None
    for marker, sentence in REFUSALS:               # and each alone
        setattr(p, marker, 1)
        assert _refusal(p) == (NotImplementedError, sentence)
        setattr(p, marker, None)


def test_keep_own_options_is_the_ten_keeps_in_one_pass(monkeypatch):
    import yaml
    from gapflow_amd import problem
    from gapflow_amd.io import read_yaml_input
    one, ten = read_yaml_input(io.StringIO(ALL_KEYS)), read_yaml_input(io.StringIO(ALL_KEYS))
    problem._keep_checkpoint_freq(ten, ALL_KEYS)
    problem._keep_probes(ten, ALL_KEYS)
    problem._keep_integrals(ten, ALL_KEYS)
    problem._keep_extrema(ten, ALL_KEYS)
    problem._keep_elastic_series(ten, ALL_KEYS)
    problem._keep_weighted(ten, ALL_KEYS, '/somewhere')
    problem._keep_statistics(ten, ALL_KEYS)
    problem._keep_regions(ten, ALL_KEYS)
    problem._keep_lines(ten, ALL_KEYS)
    problem._keep_init_from(ten, ALL_KEYS, '/somewhere')
    calls, load = [], yaml.full_load
    monkeypatch.setattr(yaml, 'full_load', lambda text: calls.append(1) or load(text))
    problem._keep_own_options(one, ALL_KEYS, '/somewhere')
    assert len(calls) == 1
    assert one == ten
    own = ('checkpoint_freq', 'probes', 'probes_pressure', 'integrals', 'integrals_sections_x', 'integrals_sections_y', 'extrema',
           'elastic_series', 'weighted_integrals', 'weights', 'statistics', 'statistics_fields', 'statistics_after', 'regions',
           'region_list', 'lines', 'line_list', 'init_from')
    assert all(k in one['options'] for k in own)
    assert one['options']['init_from'] == '/somewhere/coarse/checkpoint.gpf' and one['options']['checkpoint_freq'] == 12
    # without an options section there is nothing to set beside, checkpoint_freq included; without own keys only checkpoint_freq is set
    bare = {'grid': {}}
    problem._keep_own_options(bare, "grid: {Nx: 4}")
    assert bare == {'grid': {}}
    plain = {'options': {'silent': True}}
    problem._keep_own_options(plain, "options: {silent: True}")
    assert plain == {'options': {'silent': True, 'checkpoint_freq': 0}}
