"""The cases of the shear-thinning series' tests (tests/test_thinning_series_host.py on the CPU, tests/test_gpu_thinning_series.py
on the device) and the oracle's side of them: the per-cell integrands from oracle/closures.py, their fsum, the tolerance and the
three wrong stencils the tolerance must not hide.  No device here.

Every case is tests/test_gpu_probes.py: THINNING (Eyring, 48 x 10, D/N in x, periodic in y) with the grid, the law or the
equation of state exchanged.  Two things are chosen so that grad p MATTERS to the record (conditions (a), (b) of the host test):
  * the wall speeds.  shear_rate_avg's Couette part is (V - U) / h (stress.py passes U and V as the two wall velocities) and
    the rate is max(|Poiseuille part|, |Couette part|): with THINNING's U = 10, V = 1 the Couette part wins in every cell and
    the record would not depend on grad p at all.  U = 1, V = 0.9 lets the Poiseuille part h |grad p| / (2 mu0) win.
  * the state.  A problem starts from a uniform density, whose pressure has no gradient.  `modulate` gives every case a smooth
    density wave (relative amplitude `amp`, one period along x, a y-dependent amplitude in 2-D) on top of a compression of
    2 amp, over the whole ghosted array before _pre_run: that is the cases' INITIAL state; the stepped one is 4 to 8 steps later.
  * the compression.  THINNING's Dowson-Higginson law is stiff (C1 = 3.5e10): one rounding of s = rho / rho0 moves p by about
    2e-5 Pa whatever p is, and the device's eos_pressure forms s as rho * (1 / rho0) where the oracle divides (closures.hpp says
    so above film_pressure).  The tolerance grants the device's pressure a RELATIVE 1e-12; that covers those 2e-5 Pa only where
    |p| is well above 2e7 Pa.  Around the ambient pressure, where a wave about rho0 has its steepest flank and so its rate_max, it
    does not: there the two roundings alone, both taken from the oracle on the CPU, put a cell's rate at 2 to 5 times its
    per-cell bound.  With the compression p lies between 7e7 and 5e8 Pa everywhere, and the host test holds condition (c): the
    oracle with s formed the device's way stays within a tenth of the per-cell bound at every extremum and of the tolerance in
    every sum.
tauE = 5e4 puts the Eyring factor well below one (mu0 rate / tauE of order one)."""
import io
import math

import numpy as np

import test_gpu_probes as tp

EPS = 2.0 ** -52
SUMS = ('load', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top', 'tau0_xz_bot', 'tau0_yz_bot', 'tau0_xz_top', 'tau0_yz_top',
        'eta_sum', 'rate_sum')
EXTREMA = ('eta_min', 'eta_max', 'rate_max')
NAMES = SUMS + EXTREMA
GRADIENT_SUMS = ('tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top', 'eta_sum', 'rate_sum')    # the sums grad p enters

BASE = tp.THINNING.replace('U: 10., V: 1.', 'U: 1., V: 0.9').replace('tauE: 5.e5', 'tauE: 5.e4')
assert BASE != tp.THINNING and 'tauE: 5.e4' in BASE
GRID = "Nx: 48, Ny: 10, Lx: 0.05, Ly: 0.01"
PX = "xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007"
STRIDED_LAW = "    P0: 1.e8\n    C1: 3.5e8\n"
ROELANDS = "    piezo: {name: Roelands, mu_inf: 1.e-3, p_ref: 1.96e8, z: 0.68}\n"


def _case(grid=None, bc=None, law=None, piezo='', eos=None):
    t = BASE
    if grid:
        t = t.replace(GRID, grid)
    if bc is not None:
        t = t.replace(PX, bc)
    if law:
        t = t.replace('{name: Eyring, tauE: 5.e4}', law)
    if eos:
        t = t.replace('    EOS: DH\n', eos[0]).replace('    rho0: 877.7007\n', eos[1]).replace('877.7007', eos[2])
    assert t != BASE or not (grid or bc is not None or law or eos)
    return t + piezo


# name: (input, steps, relative amplitude of the density wave, slip-length field)
CASES = {
    'eyring-48x10': (_case(), 6, 1e-3, False),
    'carreau-16x1': (_case(grid="Nx: 16, Ny: 1, Lx: 0.05, Ly: 1.", law='{name: Carreau, mu_inf: 1.e-3, lam: 1.e-5, a: 2., N: 0.6}'), 8, 1e-3, False),
    # Ny = 601 > 512 and odd: a thread walks on to a second pair, the last pair is half a pair (test_gpu_integrals.STRIDED's shape)
    # and its law: P0 = 1e8, C1 = 3.5e8, under which Roelands' viscosity is 3.5 times the ambient one
    'eyring-roelands-6x601': (_case(grid="Nx: 6, Ny: 601, Lx: 0.0015, Ly: 0.12", piezo=STRIDED_LAW + ROELANDS), 4, 1e-3, False),
    # 150 pairs: three waves, the third partly filled; periodic in x: rows 1 and Nx read ghost rows that hold interior values
    'eyring-24x300-px': (_case(grid="Nx: 24, Ny: 300, Lx: 0.006, Ly: 0.06", bc="xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']"), 4, 1e-3, False),
    'eyring-slip-16x41': (_case(grid="Nx: 16, Ny: 41, Lx: 0.004, Ly: 0.01"), 5, 1e-3, True),
    'eyring-mt-20x13': (_case(grid="Nx: 20, Ny: 13, Lx: 0.05, Ly: 0.01", eos=('    EOS: MT\n', '    rho0: 700.\n', '700.')), 6, 2e-3, False),
}
CASE_NAMES = list(CASES)


def inputs(name):
    from gapflow_amd.io import read_yaml_input
    with io.StringIO(CASES[name][0]) as f:
        return read_yaml_input(f)


def slip_field(grid):
    """tests/test_gpu_integrals.py: SLIP_FIELD's per-cell slip length"""
    x = np.linspace(0., 1., grid['Nx'] + 2)[:, None]
    y = np.linspace(0., 1., grid['Ny'] + 2)[None, :]
    return 1.e-6 * (1. + np.sin(3. * x) * np.cos(2. * y))


def modulate(q, amp):
    """The cases' initial state: the density of the (uniform) ghosted state q times 1 + amp * (2 + wave), in place."""
    nx, ny = q.shape[1] - 2, q.shape[2] - 2
    X = np.arange(nx + 2)[:, None] / (nx + 1.)
    Y = np.arange(ny + 2)[None, :] / (ny + 1.)
    wave = np.sin(2 * np.pi * X + 0.3) * ((1. + 0.5 * np.cos(2 * np.pi * Y + 0.7)) if ny > 1 else np.ones_like(Y))
    q[0] *= 1. + amp * (2. + wave)
    return q


def build_oracle(name):
    """The oracle's problem of a case in its initial state, _pre_run done."""
    from oracle.problem import OracleProblem
    d = inputs(name)
    _, _, amp, slip = CASES[name]
    o = OracleProblem(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'],
                      extra_field=slip_field(d['grid']) if slip else None)
    modulate(o.q, amp)
    o._pre_run()
    return o


def full_prop(prop):
    from gapflow_amd import _lib
    return dict(_lib.EOS_DEFAULTS[prop['EOS']], **prop)


def sign_pattern(shape):
    """s = sx(ix) sy(iy) with sx, sy the pattern + + - - of period 4: the two cells of every central difference carry opposite signs"""
    s = np.array([1., 1., -1., -1.])
    return s[np.arange(shape[0]) % 4][:, None] * s[np.arange(shape[1]) % 4][None, :]


def terms(q, topo, Ls, prop, geo, grid, p_factor=None, stencil=None):
    """name -> the per-cell integrand over the interior (NAMES' sums; 'eta', 'rate' per cell beside them), from oracle/closures.py
    on the ghosted planes: eos_pressure, np.gradient over the ghosted pressure, piezoviscosity, shear_rate_avg,
    shear_thinning_factor, stress_bottom / stress_top.  p_factor: the ghosted pressure is multiplied by it (the conditioning
    allowance).  stencil: None, or one of the wrong ones -- 'zero' (grad p = 0), 'swap' (the two axes exchanged: the difference along x
    divided by 2 dy and the one along y by 2 dx -- dpx and dpy enter the record through hypot(dpx, dpy) alone, which is symmetric,
    so handing the two right values on in the wrong order is no error and cannot show; the spacing is what an exchanged stencil gets
    wrong, and every 2-D case has dx != dy), 'shift' (each difference taken one cell further on)."""
    from oracle import closures as ocl
    prop = full_prop(prop)
    U, V, zeta = geo['U'], geo['V'], prop['bulk']
    dx, dy = grid['dx'], grid['dy']
    pr = ocl.eos_pressure(q[0], prop)
    load = pr
    if p_factor is not None:
        pr = pr * p_factor
        load = pr
    dpx = np.gradient(pr, dx, axis=0)
    dpy = np.gradient(pr, dy, axis=1)
    if stencil == 'zero':
        dpx, dpy = 0. * dpx, 0. * dpy
    elif stencil == 'swap':
        dpx, dpy = np.gradient(pr, dy, axis=0), np.gradient(pr, dx, axis=1)
    elif stencil == 'shift':
        dpx, dpy = np.roll(dpx, -1, axis=0), np.roll(dpy, -1, axis=1)
    mu0 = prop['shear']
    if 'piezo' in prop:
        from gapflow_amd import _lib
        pz = dict(_lib.PIEZO_DEFAULTS[prop['piezo']['name']], **prop['piezo'])
        mu0 = ocl.piezoviscosity(pr if prop['EOS'] != 'Bayada' else q[0], prop['shear'], pz)
    mu0 = np.broadcast_to(mu0, pr.shape)
    rate = ocl.shear_rate_avg(dpx, dpy, topo[0], U, V, mu0)
    eta = mu0 * ocl.shear_thinning_factor(rate, mu0, prop['thinning'])
    bot, top = ocl.stress_bottom(q, topo, U, V, eta, zeta, Ls), ocl.stress_top(q, topo, U, V, eta, zeta, Ls)
    bot0, top0 = ocl.stress_bottom(q, topo, U, V, mu0, zeta, Ls), ocl.stress_top(q, topo, U, V, mu0, zeta, Ls)
    out = dict(load=load, tau_xz_bot=bot[4], tau_yz_bot=bot[3], tau_xz_top=top[4], tau_yz_top=top[3], tau0_xz_bot=bot0[4],
               tau0_yz_bot=bot0[3], tau0_xz_top=top0[4], tau0_yz_top=top0[3], eta_sum=eta, rate_sum=rate, eta=eta, rate=rate)
    return {k: np.ascontiguousarray(np.broadcast_to(v, pr.shape)[1:-1, 1:-1]) for k, v in out.items()}


def oracle_record(q, topo, Ls, prop, geo, grid, stencil=None):
    """What the record is held to, from the oracle alone: name -> (value, tolerance) for the eleven sums -- fsum of the terms
    times dx dy; the film integrals' (1e-12 + n eps) sum|term| dA plus twice the conditioning allowance sum|term(p (1 + 1e-12 s))
    - term(p)| dA --, `allowance` and `magnitude` (sum|term| dA) per name, and per cell eta, rate with their per-cell bounds
    (1e-12 + 4 eps) |value| + 2 |value(p (1 + 1e-12 s)) - value(p)|."""
    dA = grid['dx'] * grid['dy']
    t = terms(q, topo, Ls, prop, geo, grid, stencil=stencil)
    moved = terms(q, topo, Ls, prop, geo, grid, p_factor=1. + 1e-12 * sign_pattern(q[0].shape), stencil=stencil)
    out = {'value': {}, 'tol': {}, 'allowance': {}, 'magnitude': {}}
    for n in SUMS:
        v = t[n].ravel()
        mag = math.fsum(np.abs(v)) * dA
        allow = math.fsum(np.abs(moved[n].ravel() - v)) * dA
        out['value'][n], out['magnitude'][n], out['allowance'][n] = math.fsum(v) * dA, mag, allow
        out['tol'][n] = (1e-12 + v.size * EPS) * mag + 2. * allow
    for n in ('eta', 'rate'):
        out[n] = t[n]
        out[n + '_bound'] = (1e-12 + 4 * EPS) * np.abs(t[n]) + 2. * np.abs(moved[n] - t[n])
    return out


def _oracle_pressure(rho, prop):
    from oracle import closures as ocl
    return getattr(ocl.eos_pressure, 'oracle_own', ocl.eos_pressure)(rho, prop)


def device_form_pressure(rho, prop):
    """oracle/closures.py: eos_pressure with s formed as the device's eos_pressure<EOS_DH> forms it, rho * (1 / rho0) with the
    reciprocal rounded once, where the oracle divides; the other laws as they are."""
    if prop['EOS'] != 'DH':
        return _oracle_pressure(rho, prop)
    s = np.minimum(rho, 0.99 * prop['C2'] * prop['rho0']) * (1.0 / prop['rho0'])
    return prop['P0'] + prop['C1'] * (s - 1.0) / (prop['C2'] - s)


def device_form_terms(q, topo, Ls, prop, geo, grid):
    """terms() with device_form_pressure in eos_pressure's place"""
    from oracle import closures as ocl
    real = ocl.eos_pressure
    device_form_pressure.oracle_own = real
    ocl.eos_pressure = device_form_pressure
    try:
        return terms(q, topo, Ls, prop, geo, grid)
    finally:
        ocl.eos_pressure = real


def oracle_record_of(o, stencil=None):
    """oracle_record of an OracleProblem's (or a device Problem's downloaded) current state"""
    if hasattr(o, 'extra'):
        return oracle_record(o.q, o.topo[:3], o.extra[0], o.prop, o.geo, o.grid, stencil)
    return oracle_record(np.array(o.q), np.array(o.topo.full[:3]), np.array(o._extra[0]), o.prop, o.geo, o.grid, stencil)
