"""Checkpoint and restart (gpf_checkpoint_*, Problem.save_checkpoint / from_checkpoint, SlabProblem, options.checkpoint_freq).

The property of every case: run A does n1 steps, saves, does n2 more; run B is built from the file in a fresh Problem and does
n2 steps.  A and B then agree in every bit: q with its ghost cells, every member of gpf_scalars_t of each of the n2 steps, step,
converged, residual_buffer -- and pressure / bulk stress / wall stress read from B right after the load, before any step, equal
what A held at the save (the corrector-stage closures: they need the previous buffer and dt_last, or the saved derived planes).
Reference: none (the reference has no restart); the yardstick is the uninterrupted run itself, bit for bit,
because both runs execute the same kernels on the same bits in the same order."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N1, N2 = 7, 9           # an odd step count at the save: the second q buffer is the current one, MC_order 0 sweeps backwards next
SCALARS = ('step', 'simtime', 'dt', 'ekin', 'ekin_old', 'residual', 'v_max', 'v_sound', 'mass', 'invalid', 'converged')

JOURNAL_1D = """
options: {silent: True}
grid: {Nx: 100, Ny: 1, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}
"""

# 70 x 130: more than 1200 cells (k_step2), one full 126-column strip and a ragged one, 70 rows is no multiple of 8
GRID_2D = "Nx: 70, Ny: 130, Lx: 0.02, Ly: 0.03, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: {rho0}, xW_D: {rho0}, yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']"
TWO_D = """
options: {{silent: True}}
grid: {{""" + GRID_2D + """}}
geometry: {geo}
numerics: {{CFL: 0.4, adaptive: {adaptive}, MC_order: {mc}, tol: 1e-14, dt: 2.e-9, max_it: 100000}}
properties: {prop}
"""
INCLINED = "{type: inclined, hmax: 1.2e-5, hmin: 4.e-6, U: 0.5, V: 0.}"
ASPERITY = "{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.05}"
DH = "{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}"
BAYADA_DUKLER = "{EOS: Bayada, rho0: 850., shear: 0.039, bulk: 0., cl: 1600., cv: 352., piezo: {name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}}"
PL = "{EOS: PL, shear: 1.846e-5, bulk: 0., rho0: 1.1853, P0: 101325., alpha: 0.}"


def two_d(geo=INCLINED, prop=DH, rho0=877.7007, mc=0, adaptive=1):
    return TWO_D.format(geo=geo, prop=prop, rho0=rho0, mc=mc, adaptive=adaptive)


# tests/test_gpu_extras.py: THINNING (Eyring, 48 x 10), restated
THINNING = """
options: {silent: True}
grid: {Nx: 48, Ny: 10, Lx: 0.05, Ly: 0.01, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: parabolic, hmin: 1.e-5, hmax: 4.e-5, U: 10., V: 1.}
numerics: {CFL: 0.4, adaptive: 1, max_it: 100}
properties:
    EOS: DH
    shear: 0.05
    bulk: 0.
    rho0: 877.7007
    thinning: {name: Eyring, tauE: 5.e5}
"""

# tests/test_gpu_elastic.py: BASE with CASES['example_1d'] (examples/config/parabolic_1d_elastic.yaml), restated
ELASTIC = """
options: {silent: True}
grid: {Lx: 0.0762, Ly: 1., Nx: 100, Ny: 1, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 850., xW_D: 850., yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: parabolic, hmin: 2.54e-5, hmax: 5.08e-5, U: 4.57, V: 0.}
numerics: {adaptive: 1, CFL: 0.45, tol: 1e-8, dt: 1.e-10, max_it: 60}
properties:
    EOS: Bayada
    rho0: 850.
    shear: 0.039
    bulk: 0.
    cl: 1600.
    cv: 352.
    elastic: {E: 50e09, v: 0.3, alpha_underrelax: 1e-3}
    piezo: {name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}
"""


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def scalars_of(p):
    sc = p._scalars()
    return tuple(getattr(sc, k) for k in SCALARS)


def steps(p, n):
    """n single updates; the full gpf_scalars_t after each."""
    out = []
    for _ in range(n):
        p.update()
        out.append(scalars_of(p))
    return out


def closures_of(p):
    return (np.array(p.pressure.pressure), np.array(p.bulk_stress.stress), np.array(p.wall_stress_xz.full))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bitwise(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    same = bits(a) == bits(b)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ, max |difference| {np.nanmax(np.abs(a - b)):.3e}"


def assert_same_scalars(la, lb):
    assert len(la) == len(lb)
    for i, (ra, rb) in enumerate(zip(la, lb)):
        for k, x, y in zip(SCALARS, ra, rb):
            if isinstance(x, float):
                assert bits(x) == bits(y), f"step {i + 1} after the load: {k} {x!r} vs {y!r}"
            else:
                assert x == y, f"step {i + 1} after the load: {k} {x!r} vs {y!r}"


def build(text, extra=None, device=0):
    from gapflow_amd import Problem
    from gapflow_amd.io import read_yaml_input
    if extra is None:
        return quiet(Problem.from_string, text, device)
    d = quiet(read_yaml_input, io.StringIO(text))
    return quiet(Problem, d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'], extra_field=extra, device=device)


def interrupted_and_restarted(text, path, extra=None, closures_before_save=False, destroy_a_first=False, n1=N1, n2=N2):
    """-> (A, B, closures A held at the save, closures of B right after the load); the bitwise property asserted."""
    from gapflow_amd import Problem
    a = build(text, extra)
    a._pre_run()
    steps(a, n1)
    if closures_before_save:
        at_save = closures_of(a)            # (the handle then no longer keeps the previous state: the blob carries the derived planes)
        a.save_checkpoint(path)
    else:
        a.save_checkpoint(path)
        at_save = closures_of(a)
    log_a = steps(a, n2)
    qa, fin_a = np.array(a.q), (a.step, a.converged, list(a.residual_buffer), a.simtime, a.dt, a.residual)
    if destroy_a_first:
        a.__del__()
    b = quiet(Problem.from_checkpoint, path)
    assert b.step == n1
    after_load = closures_of(b)
    for name, x, y in zip(('pressure', 'bulk stress', 'wall stress xz'), at_save, after_load):
        assert_bitwise(x, y, f'{name} right after the load')
    log_b = steps(b, n2)
    assert_bitwise(qa, b.q, 'q after the continued run')
    assert_same_scalars(log_a, log_b)
    assert fin_a[0] == b.step and fin_a[1] == b.converged
    assert_bitwise(fin_a[2], list(b.residual_buffer), 'residual_buffer')
    assert_bitwise(fin_a[3:], (b.simtime, b.dt, b.residual), 'simtime, dt, residual of the host mirror')
    return a, b, at_save, after_load


def test_journal_1d_through_the_small_grid_kernel(hiplib, tmp_path):
    """Nx = 100, Ny = 1, periodic, adaptive CFL 0.25: k_small_steps.  A's handle is destroyed before B is built."""
    interrupted_and_restarted(JOURNAL_1D, str(tmp_path / 'c.gpf'), destroy_a_first=True)


CHILD = '''
import sys, io, contextlib, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_checkpoint as T
from gapflow_amd import Problem
own, other, out = sys.argv[1:4]
a, b, _, _ = T.interrupted_and_restarted(T.JOURNAL_1D, own)          # this form against itself, bitwise
with contextlib.redirect_stdout(io.StringIO()):
    x = Problem.from_checkpoint(other)                                # the other form's file
    q0, sc0 = np.array(x.q), T.scalars_of(x)
    x.save_checkpoint(out + '.resaved')
    logx = T.steps(x, T.N2)
    y = Problem.from_checkpoint(other)
    logy = T.steps(y, T.N2)
T.assert_bitwise(x.q, y.q, 'two continuations of the other form\\'s file')
T.assert_same_scalars(logx, logy)
with contextlib.redirect_stdout(io.StringIO()):
    z = Problem.from_checkpoint(own)                                  # what THIS form saved, for the parent to load
np.savez(out, q0=q0, sc0=np.array(sc0, dtype=float), qx=x.q, dt=x.dt, simtime=x.simtime, q_own=z.q, sc_own=np.array(T.scalars_of(z), dtype=float))
'''


def test_journal_1d_through_k_step2_and_across_the_two_forms(hiplib, tmp_path):
    """GPF_SMALL_GRID=0 in a child process (the switch is read once per process): the same problem through k_step2 at a tiny
    size, bitwise against itself; and the file written by the small-grid form here loads into the k_step2 form there: the state
    that arrives is bitwise the saved one, the blob saved again from the other form is byte for byte the one it loaded, and
    continuing from it is reproducible.  (The two forms sum in different orders -- tests/test_gpu_extras.py holds them to 1e-10
    of each other after 77 steps -- so the continuation in the OTHER form is compared with the uninterrupted run of THIS form to
    that bound, not bitwise: there is no uninterrupted run that changes form at step 7.)"""
    import subprocess
    import sys
    from gapflow_amd import checkpoint
    here = os.path.dirname(os.path.abspath(__file__))
    small = str(tmp_path / 'small.gpf')
    a = build(JOURNAL_1D)
    a._pre_run()
    steps(a, N1)
    a.save_checkpoint(small)
    q_save, sc_save = np.array(a.q), scalars_of(a)
    steps(a, N2)
    out = str(tmp_path / 'child.npz')
    res = subprocess.run([sys.executable, '-c', CHILD % dict(root=os.path.dirname(here), tests=here), str(tmp_path / 'step2.gpf'), small, out],
                         env=dict(os.environ, GPF_SMALL_GRID='0'), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(out)
    assert_bitwise(q_save, got['q0'], 'the state the other form received')
    assert_bitwise(np.array(sc_save, dtype=float), got['sc0'], 'the scalars the other form received')
    assert checkpoint.read_file(small)[1] == checkpoint.read_file(out + '.resaved')[1], 'the blob depends on the kernel form'
    for c in range(3):
        assert np.abs(got['qx'][c] - a.q[c]).max() <= 1e-10 * np.abs(a.q[c]).max(), c
    np.testing.assert_allclose(got['dt'], a.dt, rtol=1e-13)
    # the other direction: the k_step2 form's file into the small-grid form of this process
    from gapflow_amd import Problem
    back = quiet(Problem.from_checkpoint, str(tmp_path / 'step2.gpf'))
    assert_bitwise(got['q_own'], back.q, 'the state this form received from the k_step2 form')
    assert_bitwise(got['sc_own'], np.array(scalars_of(back), dtype=float), 'the scalars this form received')
    back.save_checkpoint(str(tmp_path / 'back.gpf'))
    assert checkpoint.read_file(str(tmp_path / 'step2.gpf'))[1] == checkpoint.read_file(str(tmp_path / 'back.gpf'))[1]
    twin = quiet(Problem.from_checkpoint, str(tmp_path / 'step2.gpf'))
    assert_same_scalars(steps(back, N2), steps(twin, N2))
    assert_bitwise(back.q, twin.q, 'two continuations of the k_step2 form\'s file')


@pytest.mark.parametrize('mc,adaptive', [(0, 1), (-1, 0)], ids=['alternating-sweeps', 'backward-sweep-fixed-dt'])
def test_inclined_2d_row_coefficient_table(hiplib, tmp_path, mc, adaptive):
    """70 x 130, D/N/N in x, periodic in y, x-only gap (TOPO 4 with the table, rebuilt by the load)."""
    from gapflow_amd import _lib
    a, b, _, _ = interrupted_and_restarted(two_d(mc=mc, adaptive=adaptive), str(tmp_path / 'c.gpf'))
    n = 8 * (70 + 2 + 4)
    ta, tb = np.empty(n), np.empty(n)
    _lib.check(a._lib.gpf_row_coefficients(a._h, 0, _lib.as_dp(ta), n))
    _lib.check(b._lib.gpf_row_coefficients(b._h, 0, _lib.as_dp(tb), n))
    assert_bitwise(ta, tb, 'row-coefficient table')


def test_asperity_2d_gap_planes(hiplib, tmp_path):
    interrupted_and_restarted(two_d(geo=ASPERITY), str(tmp_path / 'c.gpf'))


def test_closures_read_before_the_save(hiplib, tmp_path):
    """Reading the closures BEFORE the save spends the previous buffer (gpf_update_closures runs the predictor in it): the blob
    then carries the derived planes instead."""
    interrupted_and_restarted(two_d(geo=ASPERITY), str(tmp_path / 'c.gpf'), closures_before_save=True)


@pytest.mark.parametrize('edit', ['q', 'gap'])
def test_edit_after_reading_the_closures(hiplib, tmp_path, edit):
    """Step, read the closures, edit q (or the gap), save: the derived planes on the device belong to the state before the edit
    and must not travel.  Both runs then form the closures of the edited state."""
    from gapflow_amd import Problem
    path = str(tmp_path / 'c.gpf')
    a = build(two_d(geo=ASPERITY))
    a._pre_run()
    steps(a, N1)
    before = closures_of(a)
    if edit == 'q':
        a.q[0, 5:20, 7:90] *= 1.001
    else:
        a.topo.h = a.topo.h * 1.01
    a.save_checkpoint(path)
    at_save = closures_of(a)
    assert not np.array_equal(before[0], at_save[0])
    b = quiet(Problem.from_checkpoint, path)
    for name, x, y in zip(('pressure', 'bulk stress', 'wall stress xz'), at_save, closures_of(b)):
        assert_bitwise(x, y, f'{name} right after the load')
    assert_same_scalars(steps(a, 3), steps(b, 3))
    assert_bitwise(a.q, b.q, 'q after the continued run')


def test_slip_length_field(hiplib, tmp_path):
    """The erf profile of tests/test_gpu_examples.py (slip example), broadcast over y, scaled to a micrometre."""
    from scipy.special import erf
    nx, ny = 70, 130
    slip = np.zeros(nx)
    e = erf(np.linspace(-20., 20., nx // 2))
    slip[:nx // 2], slip[nx // 2:] = e, -e
    slip = (1. + np.roll(slip, nx // 4)) / 2.
    extra = np.zeros((1, nx + 2, ny + 2))
    extra[0, 1:-1, :] = 1.e-6 * slip[:, None]
    extra[0, 0, :], extra[0, -1, :] = extra[0, -2, :], extra[0, 1, :]
    a, b, _, _ = interrupted_and_restarted(two_d(), str(tmp_path / 'c.gpf'), extra=extra)
    assert_bitwise(extra, b._extra, 'slip length field of the restored problem')


@pytest.mark.parametrize('prop,rho0', [(BAYADA_DUKLER, 850.), (PL, 1.1853)], ids=['bayada-dukler', 'power-law'])
def test_other_equations_of_state(hiplib, tmp_path, prop, rho0):
    interrupted_and_restarted(two_d(prop=prop, rho0=rho0), str(tmp_path / 'c.gpf'))


def test_eyring_thinning_stage_wise(hiplib, tmp_path):
    interrupted_and_restarted(THINNING, str(tmp_path / 'c.gpf'))


def test_elastic_gap(hiplib, tmp_path):
    from gapflow_amd import Problem
    path = str(tmp_path / 'c.gpf')
    a = build(ELASTIC)
    a._pre_run()
    steps(a, N1)
    a.save_checkpoint(path)
    h_a, u_a = np.array(a.topo.h), np.array(a.topo.deformation)
    assert np.abs(u_a).max() > 0
    b = quiet(Problem.from_checkpoint, path)
    assert_bitwise(h_a, b.topo.h, 'deformed gap right after the load')
    assert_bitwise(u_a, b.topo.deformation, 'deformation right after the load')
    a2, b2, _, _ = interrupted_and_restarted(ELASTIC, path)
    assert_bitwise(a2.topo.h, b2.topo.h, 'deformed gap after the continued run')
    assert_bitwise(a2.topo.deformation, b2.topo.deformation, 'deformation after the continued run')


# Chosen with the oracle (oracle/problem.py, CPU): on the 1-D journal problem the residual starts near zero and the oracle meets
# any tolerance >= 1e-4 at step 5, before a save "five steps earlier" exists; this 1-D parabolic slider's residual rises first
# (step 5: 3.8e-3) and the oracle meets tol 3e-3 at step 110 (residual 3.008e-3 at step 105, 2.737e-3 at step 106).
CONVERGING = """
options: {silent: True}
grid: {Nx: 64, Ny: 1, Lx: 0.05, Ly: 1., xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: parabolic, hmin: 1.e-5, hmax: 4.e-5, U: 10., V: 0.}
numerics: {CFL: 0.4, adaptive: 1, tol: 3.e-3, max_it: 400}
properties: {EOS: DH, shear: 0.05, bulk: 0.01, rho0: 877.7007}
"""
CONVERGED_AT = 110


def test_convergence_across_a_save(hiplib, tmp_path):
    """A run that converges shortly after the save stops at the same step when restarted: the residual ring travels.  The save
    is five steps before the oracle's convergence step (110: outside the 20 to 60 steps first aimed at -- see above -- and still
    a fraction of a second on a 64-cell problem)."""
    from gapflow_amd import Problem
    path = str(tmp_path / 'c.gpf')
    a = build(CONVERGING)
    a._pre_run()
    a._advance(CONVERGED_AT - 5, honor_stop=True)
    assert a.step == CONVERGED_AT - 5 and not a.converged
    a.save_checkpoint(path)
    quiet(a.run, keep_open=True)
    assert a.step == CONVERGED_AT and a.converged
    b = quiet(Problem.from_checkpoint, path)
    assert not b.converged
    quiet(b.run, keep_open=True)
    assert b.step == CONVERGED_AT and b.converged
    assert_bitwise(a.q, b.q, 'q at convergence')
    assert_bitwise(list(a.residual_buffer), list(b.residual_buffer), 'residual_buffer')


THINNING_SLAB = THINNING


@pytest.mark.parametrize('case', ['fused', 'thinning'])
def test_two_thread_ranks_all_gather(hiplib, tmp_path, case):
    """Two SlabProblems (threads of this process, tests/test_gpu_eight_slabs.py's pattern) save at step 7 and two fresh ones
    load and continue: bitwise the uninterrupted slab run, and the rows equal the undivided problem continued from its own file."""
    import torch
    from gapflow_amd import Problem
    from gapflow_amd.slab import SlabProblem, ThreadWorld
    text = two_d() if case == 'fused' else THINNING_SLAB       # thinning: the stage-wise slab step and its rows beyond the halo
    path = str(tmp_path / 'slab.gpf')

    def run_a(group):
        s = SlabProblem.from_string(text, device=0, dist=group)
        s.pre_run()
        s.advance(N1)
        s.save_checkpoint(path)
        s.advance(N2)
        return s.layout, s.local_q(), s.state()

    def run_b(group):
        s = SlabProblem.from_checkpoint(path, device=0, dist=group)
        assert int(s.state().step) == N1
        s.advance(N2)
        return s.layout, s.local_q(), s.state()

    ra = quiet(ThreadWorld(2, torch).run, run_a)
    assert sorted(os.listdir(tmp_path)) == ['slab.gpf.rank000', 'slab.gpf.rank001']
    rb = quiet(ThreadWorld(2, torch).run, run_b)
    serial = None
    if case == 'fused':         # (the stage-wise slab step is held to 1e-11 of the undivided one elsewhere, not bitwise)
        _, serial, _, _ = interrupted_and_restarted(text, str(tmp_path / 'serial.gpf'))
    for (L, qa, sa), (_, qb, sb) in zip(ra, rb):
        assert_bitwise(qa, qb, f'rank {L.rank}: rows after the continued run')
        for k in SCALARS:
            x, y = getattr(sa, k), getattr(sb, k)
            assert (bits(x) == bits(y)) if isinstance(x, float) else x == y, (L.rank, k, x, y)
        if serial is not None:
            assert_bitwise(qb, serial.q[:, L.lo - 1:L.hi + 2], f'rank {L.rank}: rows against the undivided restart')

    def wrong_world(group):
        with pytest.raises(RuntimeError, match='rank|ranks'):
            SlabProblem.from_checkpoint(path, device=0, dist=group)
        return True
    assert all(quiet(ThreadWorld(3, torch).run, wrong_world))


RUN = """
options: {{output: {out}, use_tstamp: False, write_freq: 25, checkpoint_freq: 10, silent: False}}
grid: {{Nx: 100, Ny: 1, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: {max_it}}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def test_run_writes_checkpoints_and_restart_continues_history(hiplib, tmp_path):
    """checkpoint_freq 10, write_freq 25, max_it 35: checkpoint.gpf is there and was last written at step 35; a copy taken at
    step 30 (a run to max_it 30) restarts through the command line, runs to 35 and equals the first run bitwise; its
    history.csv continues the step column without a gap or a repeat."""
    import csv
    from gapflow_amd import checkpoint
    from gapflow_amd.__main__ import main
    full = build(RUN.format(out=tmp_path / 'full', max_it=35))
    quiet(full.run)
    ck = tmp_path / 'full' / 'checkpoint.gpf'
    assert ck.exists() and not (tmp_path / 'full' / 'checkpoint.gpf.tmp').exists()
    assert checkpoint.read_file(str(ck))[0]['mirror']['step'] == 35
    part = build(RUN.format(out=tmp_path / 'part', max_it=30))
    quiet(part.run)
    copy = str(tmp_path / 'at30.gpf')
    shutil.copy(tmp_path / 'part' / 'checkpoint.gpf', copy)
    assert checkpoint.read_file(copy)[0]['mirror']['step'] == 30
    from gapflow_amd import Problem
    b = quiet(Problem.from_checkpoint, copy, options={'output': str(tmp_path / 'again')}, numerics={'max_it': 35})
    quiet(b.run)
    assert b.step == 35
    assert_bitwise(full.q, b.q, 'q at step 35')
    assert_bitwise((full.simtime, full.dt, full.residual), (b.simtime, b.dt, b.residual), 'simtime, dt, residual')
    assert quiet(main, ['--restart', copy, '--output', str(tmp_path / 'cli'), '--max-it', '35']) == 0
    for d in ('again', 'cli'):
        with open(tmp_path / d / 'history.csv') as f:
            rows = list(csv.DictReader(f))
        assert [int(float(r['step'])) for r in rows] == [0, 25, 30, 35], d
        assert os.path.exists(tmp_path / d / 'sol.nc')
    with open(tmp_path / 'full' / 'history.csv') as f:
        last_full = list(csv.DictReader(f))[-1]
    assert float(rows[-1]['ekin']) == float(last_full['ekin']) and float(rows[-1]['time']) == float(last_full['time'])


# ---- refusals: the handle is unchanged, shown by one more step that stays bitwise that of an untouched twin ----------------------
def _refused(p, twin, path, match, exc=RuntimeError):
    with pytest.raises(exc, match=match):
        p.load_checkpoint(path)
    assert_bitwise(twin.q, p.q, 'q after the refused load')
    assert_same_scalars(steps(twin, 1), steps(p, 1))
    assert_bitwise(twin.q, p.q, 'q one step after the refused load')


@pytest.fixture(scope='module')
def saved(hiplib, tmp_path_factory):
    """One checkpoint of the 2-D inclined problem at step 7, shared and left unchanged."""
    path = str(tmp_path_factory.mktemp('ckpt') / 'ref.gpf')
    a = build(two_d())
    a._pre_run()
    steps(a, N1)
    a.save_checkpoint(path)
    return path


def _pair(text):
    out = []
    for _ in range(2):
        p = build(text)
        p._pre_run()
        steps(p, 2)
        out.append(p)
    return out


@pytest.mark.parametrize('change,field', [(('Ny: 130', 'Ny: 128'), 'Ny'), (('rho0: 877.7007}', 'rho0: 877.7007, C1: 3.4e8}'), 'eos_par'),
                                           (('xE_D: 877.7007', 'xE_D: 877.5'), 'bc_value')], ids=['Ny', 'EOS-parameter', 'boundary-value'])
def test_refuses_another_configuration(saved, change, field):
    text = two_d()
    assert change[0] in text
    p, twin = _pair(text.replace(*change))
    _refused(p, twin, saved, f"header: field '{field}'")


def _damaged(saved, tmp_path, where):
    from gapflow_amd import checkpoint
    data = bytearray(open(saved, 'rb').read())
    meta, blob = checkpoint.read_file(saved)
    start = len(data) - len(blob)
    at = {'plane': len(data) - 12345, 'header': start + 300, 'truncated': None}[where]
    if at is None:
        data = data[:len(data) - 4096]
    else:
        data[at] ^= 0x10
    path = str(tmp_path / f'{where}.gpf')
    with open(path, 'wb') as f:
        f.write(data)
    return path


@pytest.mark.parametrize('where,match', [('plane', 'digest of plane'), ('header', 'header'), ('truncated', 'truncated')])
def test_refuses_a_damaged_file(saved, tmp_path, where, match):
    p, twin = _pair(two_d())
    _refused(p, twin, _damaged(saved, tmp_path, where), match)


def test_blob_truncated_at_the_c_abi(saved):
    """gpf_checkpoint_load itself, given fewer bytes than the header announces."""
    from gapflow_amd import checkpoint, _lib
    p, twin = _pair(two_d())
    blob = bytes(checkpoint.read_file(saved)[1])
    with pytest.raises(_lib.GapflowHipError, match='truncated'):
        checkpoint.load_device_blob(p._lib, p._h, blob[:len(blob) // 2])
    with pytest.raises(_lib.GapflowHipError, match='truncated'):
        checkpoint.load_device_blob(p._lib, p._h, blob[:100])
    assert_same_scalars(steps(twin, 1), steps(p, 1))
    assert_bitwise(twin.q, p.q, 'q one step after the refused load')


@pytest.mark.parametrize('case', ['elastic', 'random-asperities'])
def test_slabs_that_are_not_saved_refuse(hiplib, tmp_path, case):
    """Two thread-ranks: an elastic slab and a slab of randomly drawn asperities (num > 1) raise NotImplementedError from save
    and load and write no file; the library itself refuses the elastic slab's handle (gpf_checkpoint_save and _load), and the
    ranks step on afterwards."""
    import warnings
    import torch
    from gapflow_amd import checkpoint, _lib
    from gapflow_amd.slab import SlabProblem, ThreadWorld
    text = ELASTIC if case == 'elastic' else two_d(geo=ASPERITY.replace('num: 1', 'num: 4'))
    match = 'elastic slabs' if case == 'elastic' else 'randomly drawn asperity heights'
    path = str(tmp_path / 'slab.gpf')

    def body(group):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            s = SlabProblem.from_string(text, device=0, dist=group)
        s.pre_run()
        s.advance(2)
        for call in (s.save_checkpoint, s.load_checkpoint):
            with pytest.raises(NotImplementedError, match=match):
                call(path)
        if case == 'elastic':
            with pytest.raises(_lib.GapflowHipError, match='elastic slabs are not saved'):
                checkpoint.device_blob(s.lib, s._h)
            with pytest.raises(_lib.GapflowHipError, match='elastic slabs are not restored'):
                checkpoint.load_device_blob(s.lib, s._h, bytes(4096))
        s.advance(1)
        return int(s.state().step)

    assert quiet(ThreadWorld(2, torch).run, body) == [3] * 2
    assert os.listdir(tmp_path) == []


def test_surrogate_problems_are_refused(hiplib, tmp_path):
    from gapflow_amd import Problem
    p = Problem.__new__(Problem)
    p.has_gp_model, p._gp_models, p.step = True, {}, 3
    with pytest.raises(NotImplementedError, match='surrogate problems'):
        p.save_checkpoint(str(tmp_path / 'x.gpf'))
    with pytest.raises(NotImplementedError, match='surrogate problems'):
        p.load_checkpoint(str(tmp_path / 'x.gpf'))
