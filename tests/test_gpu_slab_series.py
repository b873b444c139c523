"""Domain series on x-slabs (SlabProblem.set_domain_series; csrc/slab_series_kernels.hip): the film integrals and the field
extrema of the whole domain, recorded by every rank, against the UNDIVIDED handle's record of the same state -- in every bit.

The state is gathered with gather_q(), put into a serial Problem of the same input the way SlabProblem._frame does
(`w.q[...] = q`) and evaluated with film_integrals() / field_extrema(): the comparison does not depend on which kernel steps a
small serial grid.  Ranks are threads of this process on the one GPU (gapflow_amd.slab.ThreadWorld), as in
tests/test_gpu_eight_slabs.py; the grids are the smallest that reach every path: an uneven cut across a periodic seam with an
odd Ny (the ghost column), more than 256 rows (fold threads add several rows, the rank map crosses every boundary), more than
256 column pairs (the pair loop), physical x-edges with a second EOS, a world of one.  Reference: none (single process)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

JOURNAL = """
options: {{silent: True, write_freq: 1000000{more}}}
grid: {{dx: 1.e-5, dy: 1.e-5, Nx: {nx}, Ny: {ny}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.02}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: {max_it}, MC_order: 0}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""

SLIDER = """
options: {{silent: True}}
grid: {{Nx: 12, Ny: 10, Lx: 0.1, Ly: 0.05, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: {rho0}, xW_D: {rho_w},
       yS: ['D', 'N', 'N'], yN: ['D', 'N', 'N'], yS_D: {rho0}, yN_D: {rho0}}}
geometry: {{type: inclined, hmax: 6.6e-5, hmin: 1.e-5, U: 50., V: 4.}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: -1, tol: 1.e-12, max_it: 1000}}
properties: {props}
"""
SLIDER_DH = SLIDER.format(rho0=877.7007, rho_w=875., props="{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}")
SLIDER_PL = SLIDER.format(rho0=1.1853, rho_w=1.18, props="{EOS: PL, shear: 1.8e-5, bulk: 0., rho0: 1.1853, P0: 101325., alpha: 0.}")


def journal(nx, ny, max_it=1000, more=""):
    return JOURNAL.format(nx=nx, ny=ny, max_it=max_it, more=more)


def world_of(world, body):
    """body(group) on every rank of a thread world (a loopback group for a world of one); results in rank order"""
    import torch
    from gapflow_amd.slab import LoopbackGroup, ThreadWorld
    if world == 1:
        return [body(LoopbackGroup(0, 1))]
    return ThreadWorld(world, torch).run(body)


def stepwise(text, world, nsteps, **series):
    """Every rank: arm, pre_run, nsteps times advance(1) + gather_q + state -> (integrals, extrema, states, (step, time) each)"""
    def body(group):
        from gapflow_amd.slab import SlabProblem
        slab = SlabProblem.from_string(text, device=0, dist=group)
        slab.set_domain_series(**series)
        slab.pre_run()
        states, marks = [], []
        for _ in range(nsteps):
            slab.advance(1)
            states.append(slab.gather_q())
            st = slab.state()
            assert int(st.invalid) == 0
            marks.append((int(st.step), st.simtime))
        return slab.domain_integrals, slab.domain_extrema, states, marks, slab.domain_film_integrals(), slab.domain_field_extrema()
    return world_of(world, body)


class Serial:
    """The undivided handle of the same input: the records of given states"""

    def __init__(self, text, sections_x=None, sections_y=None):
        from gapflow_amd import Problem
        self.p = Problem.from_string(text)
        if sections_x is not None or sections_y is not None:
            self.p.set_integrals(1, sections_x, sections_y)         # (never stepped: the sections film_integrals() evaluates)

    def records(self, q):
        self.p.q[...] = q
        return self.p.film_integrals(), self.p.field_extrema()


def assert_same_series(a, b, what):
    assert a._fields == b._fields
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        if isinstance(x, dict):
            assert x == y, f'{what}: {name}'
        else:
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f'{what}: {name} differs'


def assert_bitwise_the_undivided_records(runs, serial, film_every, ext_every, nsteps):
    """Rank 0's series against the serial records of the gathered states; every other rank's series against rank 0's"""
    from gapflow_amd import _lib
    film, ext, states, marks, now_film, now_ext = runs[0]
    for other in runs[1:]:
        if film is not None:
            assert_same_series(other[0], film, 'integrals across ranks')
        if ext is not None:
            assert_same_series(other[1], ext, 'extrema across ranks')
        for a, b in zip(other[2], states):
            assert np.array_equal(a, b)
    refs = [serial.records(q) for q in states]
    if film_every:
        due = [k for k in range(nsteps) if (k + 1) % film_every == 0]
        assert film.step.tolist() == [marks[k][0] for k in due] == [k + 1 for k in due]
        assert film.time.tolist() == [marks[k][1] for k in due]
        for n, k in enumerate(due):
            ref = refs[k][0]
            for name in _lib.INTEGRAL_SUMS:
                assert getattr(film, name)[n] == ref[name] and getattr(film, name).dtype == np.float64, f'step {k + 1}: {name} {getattr(film, name)[n]!r} vs {ref[name]!r}'
            assert np.array_equal(film.flow_x[n], ref['flow_x']), f'step {k + 1}: flow_x {film.flow_x[n]} vs {ref["flow_x"]}'
            assert np.array_equal(film.flow_y[n], ref['flow_y']), f'step {k + 1}: flow_y {film.flow_y[n]} vs {ref["flow_y"]}'
            assert np.array_equal(film.sections_x, ref['sections_x']) and np.array_equal(film.sections_y, ref['sections_y'])
    if ext_every:
        due = [k for k in range(nsteps) if (k + 1) % ext_every == 0]
        assert ext.step.tolist() == [k + 1 for k in due] and ext.time.tolist() == [marks[k][1] for k in due]
        assert ext.cells.dtype == np.int32 and ext.cells.shape == (len(due), 7, 2)
        for n, k in enumerate(due):
            ref = refs[k][1]
            for name in _lib.EXTREMA_NAMES:
                assert getattr(ext, name)[n] == ref[name], f'step {k + 1}: {name} {getattr(ext, name)[n]!r} vs {ref[name]!r}'
                assert tuple(ext.cells[n, ext.index[name]]) == ref[name + '_cell'], f'step {k + 1}: cell of {name}'
    # the record of the current state, collective, the same on every rank: the last state's
    ref_film, ref_ext = refs[-1]
    for run in runs:
        for key, v in ref_film.items():
            assert np.array_equal(run[4][key], v), f'domain_film_integrals: {key}'
        assert run[5] == ref_ext
    return film, ext


SX, SY = [1, 5, 6, 10, 13], [2, 9]          # x-sections in all three ranks (rows 1-5 / 6-9 / 10-13), next to their boundaries


@pytest.mark.parametrize('film_every,ext_every', [(1, 3), (3, 1)])
def test_uneven_cut_across_a_periodic_seam(hiplib, film_every, ext_every):
    """13 x 9 journal bearing, all-periodic, 3 ranks of 5 / 4 / 4 rows: five single steps, every record bit for bit the undivided
    handle's of the gathered state, the same on every rank, step and time the slab's own; one advance(5) leaves the same series."""
    text = journal(13, 9)
    series = dict(integrals=film_every, extrema=ext_every, sections_x=SX, sections_y=SY)
    runs = stepwise(text, 3, 5, **series)
    film, ext = assert_bitwise_the_undivided_records(runs, Serial(text, SX, SY), film_every, ext_every, 5)
    assert len(film.step) == 5 // film_every and len(ext.step) == 5 // ext_every
    assert film.flow_x.shape == (len(film.step), 5) and film.flow_y.shape == (len(film.step), 2)

    def in_one_call(group):
        from gapflow_amd.slab import SlabProblem
        slab = SlabProblem.from_string(text, device=0, dist=group)
        slab.set_domain_series(**series)
        slab.pre_run()
        slab.advance(5)
        return slab.domain_integrals, slab.domain_extrema
    for f5, e5 in world_of(3, in_one_call):
        assert_same_series(f5, film, 'advance(5) against five advance(1)')
        assert_same_series(e5, ext, 'advance(5) against five advance(1)')


def test_row_loop_beyond_256(hiplib):
    """523 x 6 on 8 ranks of 66 / 65 rows: the fold's threads add up to three rows each, and the rank map crosses every boundary."""
    text = journal(523, 6)
    sx = [1, 66, 67, 262, 458, 459, 523]
    runs = stepwise(text, 8, 2, integrals=1, extrema=1, sections_x=sx, sections_y=[1, 6])
    assert_bitwise_the_undivided_records(runs, Serial(text, sx, [1, 6]), 1, 1, 2)


def test_pair_loop_beyond_256(hiplib):
    """8 x 1030 on 3 ranks: 515 column pairs per row, the row workgroup's threads walk up to three."""
    text = journal(8, 1030)
    runs = stepwise(text, 3, 2, integrals=1, extrema=1, sections_y=[1, 513, 1030])
    assert_bitwise_the_undivided_records(runs, Serial(text, None, [1, 513, 1030]), 1, 1, 2)


@pytest.mark.parametrize('text', [SLIDER_DH, SLIDER_PL], ids=['DH', 'PL'])
def test_physical_edges_and_a_second_eos(hiplib, text):
    """Inclined slider with Dirichlet / Neumann edges, 12 x 10 on 2 ranks (physical ghost rows on the outer ranks)."""
    runs = stepwise(text, 2, 3, integrals=1, extrema=2)
    assert_bitwise_the_undivided_records(runs, Serial(text), 1, 2, 3)


def test_world_of_one(hiplib):
    """A handle with neither halo: the domain record is Problem.film_integrals() / field_extrema() of the same state, armed or not."""
    from gapflow_amd.slab import LoopbackGroup, SlabProblem
    text = journal(20, 7)
    runs = stepwise(text, 1, 2, integrals=2, extrema=1)
    assert_bitwise_the_undivided_records(runs, Serial(text), 2, 1, 2)
    slab = SlabProblem.from_string(text, device=0, dist=LoopbackGroup(0, 1))
    slab.pre_run()
    slab.advance(3)
    assert slab.domain_integrals is None and slab.domain_extrema is None
    film, ext = Serial(text).records(slab.gather_q())
    now = slab.domain_film_integrals()              # not armed: the default sections
    assert set(now) == set(film)
    for key, v in film.items():
        assert np.array_equal(now[key], v), key
    assert slab.domain_field_extrema() == ext


def test_a_run_that_stops_on_the_device_leaves_the_records_of_its_steps(hiplib):
    """max_it = 6, advance(10, honor_stop=True), stride 1: exactly six records, of steps 1..6, on every rank."""
    text = journal(13, 9, max_it=6)

    def body(group):
        from gapflow_amd.slab import SlabProblem
        slab = SlabProblem.from_string(text, device=0, dist=group)
        slab.set_domain_series(integrals=1, extrema=1)
        slab.pre_run()
        slab.advance(10, honor_stop=True)
        return slab.domain_integrals, slab.domain_extrema, int(slab.state().step)
    for film, ext, step in world_of(3, body):
        assert step == 6
        assert film.step.tolist() == ext.step.tolist() == [1, 2, 3, 4, 5, 6]
        assert film.load.shape == (6,) and ext.cells.shape == (6, 7, 2) and np.all(np.diff(film.time) > 0)


def test_run_writes_the_files_a_serial_run_writes(hiplib, tmp_path):
    """A non-silent run() of the uneven cut for 6 steps: rank 0 writes integrals.npz / extrema.npz with a serial run's keys, dtypes
    and shapes, their arrays bit for bit the in-memory series."""
    from gapflow_amd import Problem
    opts = ", output: {out}, use_tstamp: False, silent: False"
    slab_text = journal(13, 9, max_it=6, more=opts.format(out=tmp_path / 'slab') +
                        f", domain_series: {{integrals: 1, extrema: 3, sections_x: {SX}, sections_y: {SY}}}").replace('write_freq: 1000000', 'write_freq: 4')
    serial_text = journal(13, 9, max_it=6, more=opts.format(out=tmp_path / 'serial') +
                          f", integrals: 1, integrals_sections_x: {SX}, integrals_sections_y: {SY}, extrema: 3").replace('write_freq: 1000000', 'write_freq: 4')

    def body(group):
        from gapflow_amd.slab import SlabProblem
        slab = SlabProblem.from_string(slab_text, device=0, dist=group)      # armed from options.domain_series
        slab.run()
        return slab.domain_integrals, slab.domain_extrema
    film, ext = world_of(3, body)[0]
    assert film.step.tolist() == [1, 2, 3, 4, 5, 6] and ext.step.tolist() == [3, 6]
    Problem.from_string(serial_text).run()
    for name, series in (('integrals.npz', film), ('extrema.npz', ext)):
        got, want = np.load(tmp_path / 'slab' / name), np.load(tmp_path / 'serial' / name)
        assert sorted(got.files) == sorted(want.files)
        for key in want.files:
            assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, f'{name}: {key}'
        for key, v in series._asdict().items():
            if not isinstance(v, dict):
                assert np.array_equal(got[key], v), f'{name}: {key} differs from the in-memory series'


def test_refusals_name_the_reason_before_any_step(hiplib):
    """Shear thinning, an elastic gap and surrogate closures step stage-wise on slabs: arming raises NotImplementedError that
    names the reason, on real slabs of each kind, before any step."""
    import io
    import warnings
    import torch
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.slab import LoopbackGroup, SlabProblem, ThreadWorld
    from test_gpu_elastic_slabs import _text as elastic_text
    from test_gpu_gp_large import JOURNAL_SLAB, quiet
    from test_gpu_slab import THINNING_SLAB
    thinning = THINNING_SLAB.format(law='Eyring, tauE: 5.e5', geo='parabolic, hmin: 1.e-5, hmax: 4.e-5',
                                    bc=", xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007")
    slab = SlabProblem.from_string(thinning, device=0, dist=LoopbackGroup(0, 1))
    with pytest.raises(NotImplementedError, match='domain series: shear thinning'):
        slab.set_domain_series(integrals=1)

    def elastic_rank(group):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            slab = SlabProblem.from_string(elastic_text('periodic_2d'), device=0, dist=group)
        with pytest.raises(NotImplementedError, match='domain series: an elastic gap'):
            slab.set_domain_series(extrema=1)
        with pytest.raises(NotImplementedError, match='domain series: an elastic gap'):
            slab.domain_film_integrals()
        return slab.driver.series is None
    assert ThreadWorld(2, torch).run(elastic_rank) == [True, True]

    d = quiet(read_yaml_input, io.StringIO(JOURNAL_SLAB.format(nx=32, ny=16)))
    surrogate = quiet(SlabProblem, d, device=0, dist=LoopbackGroup(0, 1))
    assert surrogate._gp_models
    with pytest.raises(NotImplementedError, match='domain series: surrogate'):
        surrogate.set_domain_series(integrals=1, extrema=1)

    plain = SlabProblem.from_string(journal(16, 8), device=0, dist=LoopbackGroup(0, 1))
    with pytest.raises(ValueError, match='at least one of the strides'):
        plain.set_domain_series()
    assert plain.domain_integrals is None and plain.driver.series is None
