"""Through-gap velocity and stress profiles on the device (models/profiles.py; csrc/profile_kernels.hip):
(a) both operators against the reference's outputs (tests/golden/leaf_profiles.npz), (b) the reference's
tests/test_analytic.py restated on them, (c) their shape and error contract, (d) Problem.gap_profiles against the operator
fed the problem's own fields, at the walls against models.viscous, with and without gradient terms, (e) a request split
through a tiny scratch equals the unsplit one bit for bit, (f) a profile between steps leaves the run unchanged."""
import io
import os

import numpy as np
import pytest

from profile_cases import cases, scale_close

pytestmark = pytest.mark.gpu

trapezoid = getattr(np, 'trapezoid', None) or np.trapz


@pytest.fixture(scope='module')
def ops():
    from gapflow_amd import _lib
    _lib.require_device()
    from gapflow_amd.models import profiles, viscous
    return profiles, viscous


# ---- (a) -----------------------------------------------------------------------------------------------------------
def test_operators_reproduce_reference_outputs(ops):
    profiles, _ = ops
    n = 0
    for key, kind, kw, ref in cases():
        got = profiles.get_stress_profiles(**kw) if kind == 'stress' else profiles.get_velocity_profiles(**kw)
        assert len(got) == ref.shape[0], key
        for c in range(ref.shape[0]):
            try:
                scale_close(got[c], ref[c], 1e-11)
            except AssertionError as e:
                raise AssertionError(f'{key}[{c}]: {e}')
        n += 1
    assert n == 60


# ---- (b) the reference's tests/test_analytic.py ---------------------------------------------------------------------
@pytest.mark.parametrize('slip, Ls', [('both', 0.), ('both', 0.5), ('top', 0.), ('top', 0.5), ('bottom', 0.), ('bottom', 0.5)])
def test_flow_rate(ops, slip, Ls):
    profiles, _ = ops
    z = np.linspace(0., 2., 10_000)
    q = np.array([1., 2., 1.])
    u, v = profiles.get_velocity_profiles(z, q, Ls=Ls, U=1., V=1., slip=slip)
    assert np.isclose(trapezoid(u, z) / 2., q[1])
    assert np.isclose(trapezoid(v, z) / 2., q[2])


@pytest.mark.parametrize('slip, Ls', [('both', 0.), ('both', 0.5), ('top', 0.), ('top', 0.5)])
def test_avg_stress(ops, slip, Ls):
    profiles, viscous = ops
    q, h = np.array([1.0, 0.75, 0.25]), np.array([1.0, 0.01, 0.01])
    z = np.linspace(0., 1., 10_000)
    xx, yy, _, _, _, xy = profiles.get_stress_profiles(z, h, q, np.zeros(3), np.zeros(3), U=1., V=1., eta=1., zeta=1., Ls=Ls,
                                                       mode=slip)
    avg = viscous.stress_avg(q, h, U=1., V=1., eta=1., zeta=1., Ls=Ls, slip=slip)
    assert np.isclose(trapezoid(xx, z) / avg[0], 1.)
    assert np.isclose(trapezoid(yy, z) / avg[1], 1.)
    assert np.isclose(trapezoid(xy, z) / avg[2], 1.)


@pytest.mark.parametrize('slip, Ls', [('both', 0.), ('both', 0.5), ('top', 0.), ('top', 0.5)])
def test_wall_stress(ops, slip, Ls):
    profiles, viscous = ops
    q, h = np.array([1.0, 0.75, 0.25]), np.array([1.0, 0.01, 0.01])
    z = np.linspace(0., 1., 10_000)
    tau = profiles.get_stress_profiles(z, h, q, np.zeros(3), np.zeros(3), U=1., V=1., eta=1., zeta=1., Ls=Ls, mode=slip)
    top = viscous.stress_top(q, h, U=1., V=1., eta=1., zeta=1., Ls=Ls, slip=slip)
    bot = viscous.stress_bottom(q, h, U=1., V=1., eta=1., zeta=1., Ls=Ls, slip=slip)
    for c in range(6):
        assert np.isclose(bot[c], tau[c][0]) and np.isclose(top[c], tau[c][-1]), c


# ---- (c) -----------------------------------------------------------------------------------------------------------
def test_shapes_and_errors(ops):
    profiles, _ = ops
    rng = np.random.default_rng(3)
    nx, ny, nz = 5, 7, 4
    q = np.stack([rng.uniform(0.9, 1.1, (nx, ny)), rng.uniform(-1, 1, (nx, ny)), rng.uniform(-1, 1, (nx, ny))])
    h = np.stack([rng.uniform(0.5, 1.0, (nx, ny)), rng.uniform(-.1, .1, (nx, ny)), rng.uniform(-.1, .1, (nx, ny))])
    g = np.zeros((3, nx, ny))
    z1 = np.linspace(0., 1., nz)
    u, v = profiles.get_velocity_profiles(z1, q[:, 0, 0])
    assert u.shape == v.shape == (nz,)
    for z in (z1[:, None, None], h[0][None] * z1[:, None, None]):
        u, v = profiles.get_velocity_profiles(z, q, Ls=0.1)
        assert u.shape == v.shape == (nz, nx, ny)
        tau = profiles.get_stress_profiles(z, h, q, g, g, Ls=np.full((nx, ny), 0.1), mode='top')
        assert len(tau) == 6 and all(t.shape == (nz, nx, ny) for t in tau)
        # the per-cell slip length field and the scalar agree
        tau_s = profiles.get_stress_profiles(z, h, q, g, g, Ls=0.1, mode='top')
        assert all(np.array_equal(a, b) for a, b in zip(tau, tau_s))
    # point inputs against a per-cell z column: one cell, the same numbers
    u_pt, _ = profiles.get_velocity_profiles(z1, q[:, 2, 3], Ls=0.2, slip='bottom')
    u_f, _ = profiles.get_velocity_profiles(np.broadcast_to(z1[:, None, None], (nz, nx, ny)) * 1.0, q, Ls=0.2, slip='bottom')
    np.testing.assert_allclose(u_f[:, 2, 3], u_pt, rtol=1e-14, atol=1e-15)
    with pytest.raises(ValueError):
        profiles.get_velocity_profiles(z1, q)                        # 1-D z with a field (nz != ny): NumPy refuses too
    with pytest.raises(ValueError):
        profiles.get_stress_profiles(z1, h, q, g, g)
    with pytest.raises(ValueError):
        profiles.get_velocity_profiles(z1, q[:, 0, 0], slip='Top')
    with pytest.raises(ValueError):
        profiles.get_stress_profiles(z1, h[:, 0, 0], q[:, 0, 0], g[:, 0, 0], g[:, 0, 0], mode='slip')


# ---- (d) Problem.gap_profiles --------------------------------------------------------------------------------------
JOURNAL_1D = """
options: {silent: True}
grid: {dx: 1.e-5, dy: 1., Nx: 100, Ny: 1, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1e-9, dt: 1e-10, max_it: 2000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325, rho0: 877.7007, T0: 323.15, C1: 3.5e10, C2: 1.23}
"""

ASPERITY_2D = """
options: {silent: True}
grid: {Nx: 40, Ny: 24, Lx: 0.01, Ly: 0.005, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 876.,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}
numerics: {CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, max_it: 100000}
properties: {EOS: DH, shear: 0.0794, bulk: 0.02, rho0: 877.7007, P0: 1.e8, C1: 3.5e8, piezo: {name: Roelands, mu_inf: 1.e-3, p_ref: 1.96e8, z: 0.68}}
"""

LARGE_DH = """
options: {silent: True}
grid: {Nx: 2048, Ny: 2048, Lx: 0.02, Ly: 0.02, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.05}
numerics: {CFL: 0.25, adaptive: 1, tol: 1e-9, dt: 1e-10, max_it: 100000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325, rho0: 877.7007, C1: 3.5e10, C2: 1.23}
"""


def make_problem(text, slip_field=False):
    import contextlib
    from gapflow_amd import Problem
    from gapflow_amd.io import read_yaml_input
    with io.StringIO(text) as f:
        d = read_yaml_input(f)
    extra = None
    if slip_field:
        g = d['grid']
        x = np.linspace(0., 1., g['Nx'] + 2)[:, None]
        y = np.linspace(0., 1., g['Ny'] + 2)[None, :]
        extra = 1.e-6 * (1. + np.sin(3. * x) * np.cos(2. * y))
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'], extra_field=extra)
        p._pre_run()
    return p


def advance(p, n):
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(n):
            p.update()


def closure_eta(p, rho):
    from gapflow_amd.models.pressure import eos_pressure
    from gapflow_amd.models.viscosity import piezoviscosity
    prop = p.prop
    if 'piezo' not in prop:
        return np.full(rho.shape, float(prop['shear']))
    arg = rho if prop['EOS'] == 'Bayada' else eos_pressure(rho, prop)
    return piezoviscosity(arg, prop['shear'], prop['piezo'])


def check_against_operators(p, res, rows, gradients):
    from gapflow_amd.models import profiles, viscous
    q = np.array(p.q[:, rows])
    h = np.array(p.topo.full[:3, rows])
    Ls = p._extra[0][rows]
    eta = closure_eta(p, q[0])
    U, V, zeta = p.geo['U'], p.geo['V'], p.prop['bulk']
    nz = res.z.shape[0]
    np.testing.assert_allclose(res.z, h[0][None] * (np.arange(nz) / (nz - 1))[:, None, None], rtol=1e-15, atol=0)
    assert np.array_equal(res.z[-1], h[0]) and np.all(res.z[0] == 0.)
    if gradients:
        full = np.array(p.q)
        dqx = (np.gradient(full, axis=1) / p.grid['dx'])[:, rows]
        dqy = np.gradient(full, axis=2)[:, rows] / p.grid['dy']
    else:
        dqx = dqy = np.zeros_like(q)
    u, v = profiles.get_velocity_profiles(res.z, q, Ls=Ls, U=U, V=V, slip='top')
    tau = profiles.get_stress_profiles(res.z, h, q, dqx, dqy, U=U, V=V, eta=eta, zeta=zeta, Ls=Ls, mode='top')
    scale_close(res.u, u, 1e-11)
    scale_close(res.v, v, 1e-11)
    for c in range(6):
        scale_close(res.tau[c], tau[c], 1e-11)
    kw = dict(U=U, V=V, eta=eta, zeta=zeta, Ls=Ls, slip='top')
    g = dict(dqx=dqx, dqy=dqy) if gradients else {}
    bot, top = viscous.stress_bottom(q, h, **kw, **g), viscous.stress_top(q, h, **kw, **g)
    for c in range(6):
        if np.any(bot[c]):
            scale_close(res.tau[c, 0], bot[c], 1e-11)
        if np.any(top[c]):
            scale_close(res.tau[c, -1], top[c], 1e-11)


@pytest.mark.parametrize('case', ['journal_1d', 'asperity_2d_slip_roelands'])
def test_problem_profiles_match_operators(case):
    p = make_problem(JOURNAL_1D) if case == 'journal_1d' else make_problem(ASPERITY_2D, slip_field=True)
    advance(p, 25)
    nxg, nyg = p.q.shape[1:]
    for gradients in (False, True):
        res = p.gap_profiles(nz=9, gradients=gradients)
        assert res.z.shape == res.u.shape == res.v.shape == (9, nxg, nyg) and res.tau.shape == (6, 9, nxg, nyg)
        check_against_operators(p, res, slice(0, nxg), gradients)
    part = p.gap_profiles(nz=9, rows=slice(3, 11), fields=('u', 'v'))
    assert part.z is None and part.tau is None and part.u.shape == (9, 8, nyg)
    full = p.gap_profiles(nz=9)
    assert np.array_equal(part.u, full.u[:, 3:11]) and np.array_equal(part.v, full.v[:, 3:11])
    for bad in (dict(nz=1), dict(rows=slice(0, nxg + 1)), dict(rows=slice(5, 5)), dict(rows=slice(0, 4, 2)), dict(fields=('w',))):
        with pytest.raises(ValueError):
            p.gap_profiles(**bad)


def test_problem_profiles_large_grid_row_slice():
    p = make_problem(LARGE_DH)
    advance(p, 3)
    rows = slice(1021, 1026)
    res = p.gap_profiles(nz=6, rows=rows, gradients=True)
    assert res.u.shape == (6, 5, 2050)
    check_against_operators(p, res, rows, True)


def test_unsupported_closures_refuse():
    text = ASPERITY_2D.replace("piezo: {name: Roelands, mu_inf: 1.e-3, p_ref: 1.96e8, z: 0.68}",
                               "thinning: {name: Eyring, tauE: 5.e5}")
    p = make_problem(text)
    with pytest.raises(NotImplementedError):
        p.gap_profiles()
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError):
        SlabProblem.gap_profiles(object())


# ---- (e) -----------------------------------------------------------------------------------------------------------
def test_split_through_tiny_scratch_is_bitwise_equal(monkeypatch):
    p = make_problem(ASPERITY_2D, slip_field=True)
    advance(p, 5)
    whole = p.gap_profiles(nz=40, gradients=True)
    monkeypatch.setenv('GPF_PROFILE_SCRATCH_MB', '0.01')       # below one row of all levels: rows and level runs both split
    split = p.gap_profiles(nz=40, gradients=True)
    monkeypatch.setenv('GPF_PROFILE_SCRATCH_MB', '1')          # a few rows at a time
    rows = p.gap_profiles(nz=40, gradients=True)
    for f in ('z', 'u', 'v', 'tau'):
        assert np.array_equal(getattr(whole, f), getattr(split, f)), f
        assert np.array_equal(getattr(whole, f), getattr(rows, f)), f


# ---- (f) -----------------------------------------------------------------------------------------------------------
def test_profiles_between_steps_leave_the_run_unchanged():
    a, b = make_problem(ASPERITY_2D, slip_field=True), make_problem(ASPERITY_2D, slip_field=True)
    advance(a, 20)
    advance(b, 10)
    b.gap_profiles(nz=16, gradients=True)
    advance(b, 10)
    assert np.array_equal(a.q, b.q)
    assert a.step == b.step and a.simtime == b.simtime and a.dt == b.dt
    assert a.history == b.history
    assert a.kinetic_energy == b.kinetic_energy and a.residual == b.residual
