"""Ensembles (gpf_ensemble_*, gapflow_amd.Ensemble): many small problems in one launch, one workgroup each.

The property of every case: a member of an ensemble is, in every bit, the same problem built afresh and advanced alone -- q with
its ghost cells, step, simtime, dt, residual_buffer, every member of gpf_scalars_t of every step, the derived fields, the files
of a run.  Reference: none (the reference has no ensembles); the yardstick is the solo run itself, bit for bit, because
k_small_ensemble and k_small_steps execute one and the same body (csrc/small_kernel.hip) on the same bits in the same order.
Shapes: the smallest that reach every path -- Nx 16 .. 100 (one to three cells per thread of the 512), a 2-D 20 x 20 member
beside 1-D ones (unequal LDS needs in one launch), three kernel instantiations and a slip-length field (several launches per
call), 300 members (more workgroups than the chip has CUs)."""
import contextlib
import csv
import ctypes as C
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALARS = ('step', 'simtime', 'dt', 'ekin', 'ekin_old', 'residual', 'v_max', 'v_sound', 'mass', 'invalid', 'converged')
PERIODIC = "xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']"
DIRICHLET = "xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: {rho0}, xW_D: {rho0}"
DH = "EOS: DH, shear: 0.0794, bulk: 0., P0: 101325., rho0: 877.7007, C1: {C1}, C2: {C2}"
PL = "EOS: PL, shear: 1.846e-5, bulk: 0., rho0: 1.1853, P0: 101325., alpha: 0."
CUBIC = "EOS: cubic, shear: 0.05, bulk: 0., rho0: 750., a: 1.33030e-1, b: -1.41778e2, c: 8.35134e4, d: -2.86532e6"


def journal(nx, eps=0.7, U=0.1, edges=PERIODIC, prop=None, adaptive=1, mc=0, dt='1e-10', cfl=0.25, tol='1e-12', max_it=100000,
            options='silent: True', ny=1, rho0=877.7007):
    prop = prop or DH.format(C1='3.5e10', C2=1.23)
    ly = 1. if ny == 1 else 0.02
    return f"""
options: {{{options}}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: 0.1, Ly: {ly}, {edges.format(rho0=rho0)}}}
geometry: {{type: journal, CR: 1.e-2, eps: {eps}, U: {U}, V: 0.}}
numerics: {{CFL: {cfl}, adaptive: {adaptive}, MC_order: {mc}, tol: {tol}, dt: {dt}, max_it: {max_it}}}
properties: {{{prop}}}
"""


# case 1: five 1-D journal bearings, Nx 24 .. 100, differing in eps, U, EOS constants, edges, fixed / adaptive dt, MC_order
FIVE = [journal(100, eps=0.7, U=0.1, mc=0),
        journal(24, eps=0.5, U=0.05, prop=DH.format(C1='3.5e9', C2=1.23), adaptive=0, dt='1e-10', mc=1),
        journal(57, eps=0.9, U=0.2, edges=DIRICHLET, mc=1),
        journal(77, eps=0.3, U=0.1, prop=DH.format(C1='3.5e10', C2=1.3), adaptive=0, dt='2e-10', mc=0),
        journal(41, eps=0.6, U=0.15, edges=DIRICHLET, cfl=0.4, mc=0)]
# case 2: three equations of state, one member with a slip-length field, one 2-D member
MIXED = [(journal(64, mc=0), False),
         (journal(33, eps=0.5, prop=PL, rho0=1.1853, edges=DIRICHLET, mc=1), False),
         (journal(48, eps=0.4, prop=CUBIC, rho0=750., mc=0), False),
         (journal(40, eps=0.6, mc=1), True),
         (journal(20, ny=20, eps=0.5, mc=0), False),
         (journal(29, eps=0.8, prop=PL, rho0=1.1853, mc=0), False)]
# case 3: three parameter sets, Nx = 16
THREE = [journal(16, eps=0.7, U=0.1), journal(16, eps=0.4, U=0.2, mc=1), journal(16, eps=0.8, U=0.05, adaptive=0, dt='1e-10')]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(text, slip=False, pre_run=True):
    from gapflow_amd import Problem
    from gapflow_amd.io import read_yaml_input

    def make():
        d = read_yaml_input(io.StringIO(text))
        extra = None
        if slip:
            g = d['grid']
            x = np.linspace(0., 1., g['Nx'] + 2)[:, None]
            y = np.linspace(0., 1., g['Ny'] + 2)[None, :]
            extra = 1.e-6 * (1. + np.sin(3. * x) * np.cos(2. * y))
        p = Problem(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'], extra_field=extra)
        if pre_run:
            p._pre_run()
        return p
    return quiet(make)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bitwise(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.size} values differ in their bits"


def records(entries):
    return [tuple(getattr(e, k) for k in SCALARS) for e in entries]


def mirror(p):
    return (p.step, p.simtime, p.dt, p.residual, tuple(p.residual_buffer))


def assert_same_records(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} records, {len(want)} from the solo run"
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0] and a[-2:] == b[-2:], f"{what}: record {k}: step / invalid / converged {a} != {b}"
        assert_bitwise(a[1:-2], b[1:-2], f"{what}: record {k}")


def assert_same_state(p, solo, what):
    assert_bitwise(p.q, solo['q'], f"{what}: q")
    got = mirror(p)
    assert got[0] == solo['mirror'][0], f"{what}: step {got[0]} != {solo['mirror'][0]}"
    assert_bitwise(got[1:4], solo['mirror'][1:4], f"{what}: simtime, dt, residual")
    assert_bitwise(got[4], solo['mirror'][4], f"{what}: residual_buffer")


_SOLO = {}


def solo(text, n, slip=False):
    """The same problem built afresh and advanced alone by n steps in one gpf_step: computed once, shared, left unchanged."""
    key = (text, n, slip)
    if key not in _SOLO:
        p = build(text, slip)
        entries = quiet(p._advance, n, honor_stop=False)
        q = p.q.copy()
        q.flags.writeable = False
        _SOLO[key] = dict(q=q, mirror=mirror(p), records=records(entries))
    return _SOLO[key]


def check_against_solo(cases, n):
    from gapflow_amd import Ensemble
    ps = [build(t, s) for t, s in cases]
    ens = Ensemble(ps)
    got = quiet(ens._advance, [n] * len(ps), honor_stop=False)
    for m, ((t, s), p) in enumerate(zip(cases, ps)):
        ref = solo(t, n, s)
        assert ref['mirror'][0] == n, f"member {m}: the solo run itself stopped at step {ref['mirror'][0]}"
        assert_same_records(records(got[m]), ref['records'], f"member {m}")
        assert_same_state(p, ref, f"member {m}")
    assert ens.steps.tolist() == [n] * len(ps)
    return ens


def test_members_equal_their_solo_runs_in_every_bit(hiplib):
    """Five 1-D journal bearings, 37 steps (odd: the batch ends on the second buffer) through Ensemble.step."""
    from gapflow_amd import Ensemble
    check_against_solo([(t, False) for t in FIVE], 37)
    ps = [build(t) for t in FIVE]
    quiet(Ensemble(ps).step, 37)                # the public call: the same bits again
    for m, (t, p) in enumerate(zip(FIVE, ps)):
        assert_same_state(p, solo(t, 37), f"step(37), member {m}")


def test_mixed_instantiations_and_shapes(hiplib):
    """DH, power law and cubic members, one with a slip-length field, one 2-D 20 x 20: four launch groups in one call, unequal
    LDS needs inside the DH group."""
    check_against_solo(MIXED, 37)


def test_more_members_than_compute_units(hiplib):
    """300 members of Nx = 16 drawn cyclically from three parameter sets, 20 steps: workgroups that follow one another on a CU."""
    from gapflow_amd import Ensemble
    ps = [build(THREE[m % 3]) for m in range(300)]
    quiet(Ensemble(ps).step, 20)
    for m, p in enumerate(ps):
        assert_same_state(p, solo(THREE[m % 3], 20), f"member {m}")


def test_members_stop_on_their_own(hiplib):
    """In one run(): a loose tol converges early, a small max_it stops on it, an absurd dt is rolled back (as
    test_invalid_state_rolls_back provokes it: a numerical rollback), one member goes the distance (max_it 150)."""
    from gapflow_amd import Ensemble
    texts = [journal(50, tol='1e-2', max_it=150), journal(64, max_it=23, mc=1), journal(40, adaptive=0, dt='1e-10', max_it=150),
             journal(72, eps=0.5, max_it=150)]

    def prepared():
        ps = [build(t) for t in texts]
        quiet(ps[2].update)
        ps[2]._lib.gpf_set_dt(ps[2]._h, 1.0)        # absurd time step -> negative densities in the next one
        ps[2].dt = 1.0
        return ps

    alone = prepared()
    for p in alone:
        quiet(p.run)
    ps = prepared()
    quiet(Ensemble(ps).run)
    for m, (p, s) in enumerate(zip(ps, alone)):
        assert_same_state(p, dict(q=s.q, mirror=mirror(s)), f"member {m}")
        assert p.history.keys() == s.history.keys()
        for k in s.history:
            assert_bitwise(p.history[k], s.history[k], f"member {m}: history['{k}']")
        assert p._stop == s._stop
    assert ps[0].converged and 5 <= ps[0].step < 150
    assert ps[1].step == 23 and not ps[1].converged
    assert ps[2]._stop and ps[2].step == 1
    assert ps[3].step == 150 and not ps[3]._stop


def test_run_writes_what_solo_runs_write(hiplib, tmp_path):
    """Two non-silent members with write_freq 10 and 25, one with checkpoint_freq 15, max_it 40: history.csv, the frames of sol.nc
    and the checkpoint are those of solo runs in other directories; the checkpoint loads and continues bitwise."""
    from scipy.io import netcdf_file
    from gapflow_amd import Ensemble, Problem, checkpoint
    opts = ["output: {out}, use_tstamp: False, write_freq: 10, silent: False",
            "output: {out}, use_tstamp: False, write_freq: 25, checkpoint_freq: 15, silent: False"]

    def members(where):
        from gapflow_amd import Problem
        return [quiet(Problem.from_string, journal(nx, eps=eps, max_it=40, options=o.format(out=tmp_path / f'{where}{k}')))
                for k, (nx, eps, o) in enumerate(zip((60, 45), (0.7, 0.5), opts))]

    alone = members('solo')
    for p in alone:
        quiet(p.run)
    ps = members('ens')
    quiet(Ensemble(ps).run)
    for k, nframes in enumerate((5, 3)):                    # steps 0 10 20 30 40; 0 25 40
        with open(tmp_path / f'solo{k}' / 'history.csv') as f:
            want = list(csv.reader(f))
        with open(tmp_path / f'ens{k}' / 'history.csv') as f:
            assert list(csv.reader(f)) == want and len(want) == nframes + 1
        with netcdf_file(str(tmp_path / f'solo{k}' / 'sol.nc'), mmap=False) as a, netcdf_file(str(tmp_path / f'ens{k}' / 'sol.nc'), mmap=False) as b:
            assert set(a.variables) == set(b.variables)
            for name in a.variables:
                assert a.variables[name].shape == b.variables[name].shape, name
                assert_bitwise(b.variables[name][:], a.variables[name][:], f"member {k}: sol.nc '{name}'")
            assert a.variables['solution'].shape[0] == nframes
    metas = [checkpoint.read_file(str(tmp_path / f'{w}1' / 'checkpoint.gpf')) for w in ('solo', 'ens')]
    assert metas[0][0]['mirror'] == metas[1][0]['mirror'] and metas[0][0]['mirror']['step'] == 40
    assert bytes(metas[0][1]) == bytes(metas[1][1]), "device blob of the checkpoint"
    cont = [quiet(Problem.from_checkpoint, str(tmp_path / f'{w}1' / 'checkpoint.gpf'), options={'silent': True}, numerics={'max_it': 51})
            for w in ('solo', 'ens')]
    for p in cont:
        quiet(p.run)
    assert cont[1].step == 51
    assert_same_state(cont[1], dict(q=cont[0].q, mirror=mirror(cont[0])), 'continued from the checkpoint')


def test_a_member_goes_on_alone(hiplib):
    """step(9), then three update() of one member alone: twelve solo steps in every bit; the derived fields and the film
    integrals right after the ensemble step are the solo ones (they need the previous-state buffer the kernel leaves)."""
    from gapflow_amd import Ensemble
    texts = [journal(64, mc=1), journal(37, eps=0.5, edges=DIRICHLET)]
    ps = [build(t) for t in texts]
    quiet(Ensemble(ps).step, 9)
    for m, (t, p) in enumerate(zip(texts, ps)):
        s = build(t)
        quiet(s._advance, 9, honor_stop=False)
        assert_bitwise(p.pressure.pressure, s.pressure.pressure, f"member {m}: pressure")
        assert_bitwise(p.wall_stress_xz.lower, s.wall_stress_xz.lower, f"member {m}: lower wall stress")
        a, b = p.film_integrals(), s.film_integrals()
        for k in b:
            assert_bitwise(a[k], b[k], f"member {m}: film_integrals()['{k}']")
        for _ in range(3):
            quiet(p.update)
        assert_same_state(p, solo(t, 12), f"member {m} after three steps alone")


def test_zero_steps_leave_a_member_untouched(hiplib):
    """n = [5, 0, 5]: the middle member's device state (both buffers, run state: its checkpoint blob) and its mirror stay."""
    from gapflow_amd import Ensemble, checkpoint
    texts = [journal(30), journal(44, eps=0.5, mc=1), journal(52, edges=DIRICHLET)]
    ps = [build(t) for t in texts]
    quiet(ps[1]._advance, 3, honor_stop=False)
    before, held = bytes(checkpoint.device_blob(ps[1]._lib, ps[1]._h)), mirror(ps[1])
    ens = Ensemble(ps)
    got = quiet(ens._advance, [5, 0, 5], honor_stop=False)
    assert got[1] == [] and ens.steps.tolist() == [5, 3, 5]
    assert bytes(checkpoint.device_blob(ps[1]._lib, ps[1]._h)) == before and mirror(ps[1]) == held
    assert_same_state(ps[1], solo(texts[1], 3), 'the member left alone')
    for m in (0, 2):
        assert_same_state(ps[m], solo(texts[m], 5), f"member {m}")


THINNING = """
options: {silent: True}
grid: {Nx: 48, Ny: 10, Lx: 0.05, Ly: 0.01, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: parabolic, hmin: 1.e-5, hmax: 4.e-5, U: 10., V: 1.}
numerics: {CFL: 0.4, adaptive: 1, max_it: 100}
properties: {EOS: DH, shear: 0.05, bulk: 0., rho0: 877.7007, thinning: {name: Eyring, tauE: 5.e5}}
"""


def _usable_alone(p):
    if p.step is None:
        quiet(p._pre_run)
    at = p.step
    quiet(p.update)
    assert p.step == at + 1 and not p._stop


def test_refusals_name_the_member(hiplib):
    from gapflow_amd import Ensemble
    good = build(journal(32))
    big = build(journal(200, ny=200), pre_run=False)
    with pytest.raises(NotImplementedError, match=r"member 1: .*200 x 200.*LDS"):
        Ensemble([good, big])
    thin = build(THINNING, pre_run=False)
    with pytest.raises(NotImplementedError, match=r"member 1: .*shear thinning"):
        Ensemble([good, thin])
    integ = build(journal(40))
    integ.set_integrals(2)
    with pytest.raises(NotImplementedError, match=r"member 0: .*integrals"):
        Ensemble([integ, good])
    probed = build(journal(40))
    probed.set_probes([[3, 1]])
    with pytest.raises(NotImplementedError, match=r"member 2: .*probes"):
        Ensemble([good, build(journal(20)), probed])
    with pytest.raises(ValueError, match=r"member 1 is the same Problem as member 0"):
        Ensemble([good, good])
    with pytest.raises(ValueError, match=r"at least one member"):
        Ensemble([])
    for p in (good, big, thin, integ, probed):
        _usable_alone(p)
    assert len(integ.integrals.step) == 0 and len(probed.probes.step) == 1     # their series went on (steps 1: odd, stride 2)


def test_library_refusals(hiplib):
    """The C ABI refuses by itself what the Python layer refuses first: GPF_ERR_INVALID (-1 .. by name) with the member and the
    reason in gpf_last_error, at create and -- for a member armed since, or not yet through gpf_pre_run -- at step."""
    from gapflow_amd import Ensemble, _lib
    lib = hiplib
    good, big, late = build(journal(32)), build(journal(200, ny=200), pre_run=False), build(journal(28), pre_run=False)

    def create(ps):
        e = C.c_void_p()
        handles = (C.c_void_p * max(len(ps), 1))(*[p._h.value for p in ps])
        return lib.gpf_ensemble_create(handles, len(ps), C.byref(e)), lib.gpf_last_error().decode(), e

    rc, msg, _ = create([good, big])
    assert rc != 0 and 'member 1' in msg and 'LDS' in msg
    rc, msg, _ = create([good, good])
    assert rc != 0 and 'member 1' in msg and 'same handle' in msg
    rc, msg, _ = create([])
    assert rc != 0 and 'at least one member' in msg
    ens = Ensemble([good, late])
    n, done = (C.c_int64 * 2)(4, 4), (C.c_int64 * 2)()
    assert lib.gpf_ensemble_step(ens._e, n, 0, done) != 0
    assert 'member 1' in lib.gpf_last_error().decode() and 'gpf_pre_run' in lib.gpf_last_error().decode()
    with pytest.raises(RuntimeError, match=r"member 1: .*_pre_run"):
        ens.step(4)
    quiet(late._pre_run)
    good.set_probes([[2, 1]])                   # armed after the ensemble was made
    assert lib.gpf_ensemble_step(ens._e, n, 0, done) != 0
    assert 'member 0' in lib.gpf_last_error().decode() and 'probes' in lib.gpf_last_error().decode()
    with pytest.raises(NotImplementedError, match=r"member 0: .*probes"):
        ens.step(4)
    assert good.step == 0 and late.step == 0    # a refused call advanced nobody
    good.clear_probes()
    quiet(ens.step, [4, 0])
    assert_same_state(good, solo(journal(32), 4), 'after the refusals')
    with pytest.raises(ValueError, match=r"4097"):
        ens._advance([4097, 0], honor_stop=False)


def test_host_limits_are_the_librarys(hiplib):
    """The three limits the host plans with (gapflow_amd/_lib.py) are what the library reports; loading checks it too."""
    from gapflow_amd import _lib
    lds, per_cell, steps = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    assert hiplib.gpf_ensemble_limits(C.byref(lds), C.byref(per_cell), C.byref(steps)) == 0
    assert (lds.value, per_cell.value, steps.value) == (_lib.SMALL_GRID_LDS_BYTES, _lib.SMALL_GRID_DOUBLES_PER_CELL, _lib.LOG_CAPACITY)
