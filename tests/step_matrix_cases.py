"""The case table of tests/test_gpu_step_matrix.py (k_step2 against the oracle) and tests/test_step_matrix_host.py (the table
against its own claims, on the oracle alone): every instantiation step2_kernel() (csrc/api.hip) can select -- seven equations of
state x {planes, slip, piezo, slip+piezo, line, y-line, coef, table} x both sweep directions.  Texts and functions only.

The property sets are those of the step_parabolic1d_* and wave_decay_cubic fixtures (Lennard-Jones-like units: Lx 1470, gap
12..60, U 0.12, shear 2.15); every grid is above the one-workgroup limit of (Nx+2)(Ny+2) = 1200 cells, so k_step2 runs it.

Shapes (rows x columns; a wavefront of k_step2 owns 126 output columns, a workgroup's four waves split the rows into chunks):
  14 x 130   two strips, the second holding 4 columns, the ghost column and its two idle lanes
  37 x 40    one partial strip; 37 rows do not divide into the row chunks
  230 x 20   with GPF_CHUNKS=2: two waves of >= 100 rows each, the load ring of the march in steady state (LONG)
"""
import contextlib
import io
import os
from collections import namedtuple

import numpy as np

STEPS = 6
SHAPES = [(14, 130), (37, 40)]
LONG_SHAPE, LONG_CHUNKS = (230, 20), 2

# EOS ids of gapflow_amd/_lib.py (gpf_config.eos), restated so that the host test needs no library
EOS_ID = {'DH': 0, 'PL': 1, 'vdW': 2, 'MT': 3, 'cubic': 4, 'BWR': 5, 'Bayada': 6}
# properties: the fixtures' own; `pow_exp`: the law's pressure or sound speed calls pow / exp / log (v_sound then to 1e-9, else
# to the 1e-11 of helpers.HISTORY_RTOL); `heavy`: Step2Weight::heavy (one wave per SIMD, the shallow load ring)
Law = namedtuple('Law', 'props rho0 pow_exp heavy')
LAWS = {
    'DH': Law('EOS: DH, rho0: 877.7007, P0: 101325., C1: 3.5e10, C2: 1.23', 877.7007, False, False),
    'PL': Law('EOS: PL, rho0: 1.1853, P0: 101325., alpha: 0.', 1.1853, True, True),
    # The fixture's state (rho0 50, M 39.948) is none the step can hold: the reference's vdW sound speed is dp / d(molar density),
    # 1000 / M = 25 times below dp / drho (sound.py, restated in oracle/closures.py), so the adaptive step is five times the
    # stable one and one ulp of density grows to 1e-6 of the momentum scale within six steps (measured on the oracle alone).
    # With M = 1000 a mole per m^3 is a kg per m^3, the two derivatives agree, and the law stays as well conditioned as the others.
    'vdW': Law('EOS: vdW, rho0: 50., M: 1000., T: 100., a: 1.355, b: 0.03201', 50., False, False),
    'MT': Law('EOS: MT, rho0: 700., P0: 0.101e6, K: 0.557e9, n: 7.33', 700., True, True),
    'cubic': Law('EOS: cubic, rho0: 762.8617, a: 1.33030e-1, b: -1.41778e2, c: 8.35134e4, d: -2.86532e6', 762.8617, False, False),
    'BWR': Law('EOS: BWR, rho0: 0.8, T: 1.0, gamma: 3.0', 0.8, True, True),
    'Bayada': Law('EOS: Bayada, rho0: 850., rho_l: 850., rho_v: 0.019, c_l: 1600., c_v: 352.', 850., True, True),
}
VARIANTS = ['planes', 'slip', 'piezo', 'slip+piezo', 'line', 'y-line', 'coef', 'table']
# (has_ls, piezo, topo) step2_kernel() must be called with
EXPECTED = {'planes': (0, 0, 0), 'slip': (1, 0, 0), 'piezo': (0, 1, 0), 'slip+piezo': (1, 1, 0), 'line': (0, 0, 1), 'y-line': (0, 0, 2),
            'coef': (0, 0, 3), 'table': (0, 0, 4), 'line-hy': (0, 0, 1)}
PIEZO_ID = {'Barus': 1, 'Roelands': 2, 'Dukler': 3, 'McAdams': 4}

Case = namedtuple('Case', 'id law variant nx ny bc piezo chunks')

TEXT = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: 1470., Ly: 1470.{bc}}}
geometry: {{type: {gap}, hmin: 12., hmax: 60., U: 0.12, V: 0.05}}
numerics: {{CFL: 0.5, adaptive: 1, dt: 1.e-3, MC_order: 0, max_it: 100}}
properties: {{{law}, shear: {shear}, bulk: 0.{piezo}}}
"""
# D/N/N on all four edges with unequal Dirichlet densities (the `dd` case of test_gpu_ragged.py, as fractions of rho0)
DD = (", xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: {0}, xW_D: {1}, yS: ['D', 'N', 'N'], yN: ['D', 'N', 'N'], yS_D: {2}, yN_D: {3}")
DD_FRACTIONS = (1., 876. / 877.7007, 877. / 877.7007, 878.5 / 877.7007)


def _pressure(law, rho):
    from oracle import closures as cl
    from oracle.config import sanitize_properties
    import yaml
    prop = sanitize_properties(yaml.full_load('{' + LAWS[law].props + ', shear: 1., bulk: 0.}'))
    return cl.eos_pressure(np.asarray(rho, float), prop)


_SPAN = {}


def pressure_span(case):
    """(p at rho0, lowest, highest pressure) of the case's final state when it runs with the constant viscosity -- what the
    constants of its piezo law are scaled to.  In these units the seven laws' pressures lie between 1 and 1e8, and the span a case
    sees is anything from 1e-4 of its pressure (power law, periodic) to several times it, zero crossing included (the stiff
    liquids between unequal Dirichlet edges): no one set of constants makes the viscosity of every case answer."""
    if case.id not in _SPAN:
        from oracle.problem import OracleProblem
        p = make(OracleProblem, case._replace(piezo=None))
        for _ in range(STEPS):
            p.update()
        pr = _pressure(case.law, p.q[0])
        _SPAN[case.id] = (float(_pressure(case.law, LAWS[case.law].rho0)), float(pr.min()), float(pr.max()))
    return _SPAN[case.id]


def piezo_text(case):
    """The `piezo:` entry and the `shear` of a piezo case: the viscosity is 2.15 at rho0 and varies by tens of per cent over
    the case's own pressure span (Barus, Roelands: a factor of 1.5 from its lowest to its highest pressure)."""
    name = case.piezo
    if case.law == 'Bayada':            # the mixture law hands its piezo law the density: alpha = (rho - rho_l) / (rho_v - rho_l)
        return f', piezo: {{name: {name}, eta_v: 1., rho_l: 850., rho_v: 800.}}', 2.15
    p0, lo, hi = pressure_span(case)
    span = hi - lo
    if name == 'Barus':                 # mu0 exp(aB p)
        aB = np.log(1.5) / span
        return f', piezo: {{name: Barus, aB: {float(aB)!r}}}', float(2.15 * np.exp(-aB * p0))
    if name == 'Roelands':              # mu0 exp(k ((1 + p / p_ref)^z - 1)), k = ln(mu0 / mu_inf); 1 + p / p_ref stays in 0.5 .. 1.5
        p_ref, z = 2. * max(abs(lo), abs(hi)), 0.68
        x0, xl, xh = (1. + v / p_ref for v in (p0, lo, hi))
        k = np.log(1.5) / (xh**z - xl**z)
        mu0 = 2.15 * np.exp(-k * (x0**z - 1.))
        return f', piezo: {{name: Roelands, mu_inf: {float(mu0 * np.exp(-k))!r}, p_ref: {p_ref!r}, z: {z}}}', float(mu0)
    # Dukler, McAdams on a pressure: the "liquid" just above the span, the "vapour" far below it -- alpha in 0.05 .. 0.16
    return f', piezo: {{name: {name}, eta_v: 0.2, rho_l: {hi + 0.5 * span!r}, rho_v: {lo - 8. * span!r}}}', 2.15


def case_text(case):
    law = LAWS[case.law]
    gap = {'planes': 'asperity', 'slip': 'asperity', 'piezo': 'asperity', 'slip+piezo': 'asperity',
           'line': 'parabolic', 'coef': 'parabolic', 'table': 'inclined', 'line-hy': 'parabolic', 'y-line': 'parabolic'}[case.variant]
    if gap == 'asperity':
        gap += ', num: 1'
    bc = DD.format(*(repr(f * law.rho0) for f in DD_FRACTIONS)) if case.bc == 'dd' else ''
    piezo, shear = piezo_text(case) if case.piezo else ('', 2.15)
    return TEXT.format(nx=case.nx, ny=case.ny, bc=bc, gap=gap, law=law.props, shear=repr(shear), piezo=piezo)


def input_of(case, reader=None):
    if reader is None:
        from oracle.config import read_yaml_input as reader
    with io.StringIO(case_text(case)) as f:
        return reader(f)


def slip_field(case, grid):
    """A smooth, periodic, non-constant slip length of 0.5 .. 3.5 (the gap is 12 .. 60), ghost cells included."""
    from oracle.topography import midpoint_grid
    x, y = midpoint_grid(grid)
    return 2. + 1.5 * np.sin(2. * np.pi * x / grid['Lx']) * np.cos(2. * np.pi * y / grid['Ly'] + 0.7)


def planes_of(case, grid):
    """Gap planes (h, dh/dx, dh/dy) the case uploads in place of its text's, for both sides the same; None: the text's own.
    y-line: the parabolic gap along y (constant along x).  line-hy: the parabolic gap along x with a dh/dy row profile that
    is not zero -- the gap stays x-only, so TOPO 1 runs with a `thy` operand that matters."""
    from oracle.topography import midpoint_grid
    if case.variant not in ('y-line', 'line-hy'):
        return None
    x, y = midpoint_grid(grid)
    s, L = (y, grid['Ly']) if case.variant == 'y-line' else (x, grid['Lx'])
    pre = 4. / L**2 * (60. - 12.)
    h, hs = pre * (s - L / 2.)**2 + 12., 2. * pre * (s - L / 2.)
    if case.variant == 'y-line':
        return np.stack([h, np.zeros_like(h), hs])
    return np.stack([h, hs, 0.02 * np.cos(2. * np.pi * x / L)])


def env_of(case):
    """Environment of the GPU run, in force from before the handle is created to after the last step."""
    env = {}
    if case.variant == 'line':          # (line-hy needs none: a row profile with dh/dy != 0 has no other kernel)
        env['GPF_TOPO_GENERIC'] = '1'
    if case.variant == 'coef':
        env['GPF_ROWCOEF_TABLE'] = '0'
    if case.chunks:
        env['GPF_CHUNKS'] = str(case.chunks)
    return env


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make(cls, case, perturb_seed=None):
    """Problem or OracleProblem of a case, after _pre_run().  perturb_seed: one ulp of relative noise on the initial density."""
    reader = None
    if cls.__module__.startswith('gapflow_amd'):
        from gapflow_amd.io import read_yaml_input as reader
    d = input_of(case, reader)
    extra = slip_field(case, d['grid']) if 'slip' in case.variant else None
    prob = cls(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'], extra_field=extra)
    planes = planes_of(case, d['grid'])
    if planes is not None:
        if hasattr(prob, '_upload_topo'):
            prob.topo.full[:3] = planes
            prob._upload_topo()
        else:
            prob.topo[:3] = planes
    prob._pre_run()
    # the initial state: the uniform one with a smooth 1 % wave on both fluxes (periodic, ghost cells included), set as the wave
    # fixtures set theirs -- with it neither flux of an x-only or y-only gap can stay where it started
    from oracle.topography import midpoint_grid
    x, y = midpoint_grid(d['grid'])
    q = prob.q.copy()
    q[1] *= 1. + 0.01 * np.cos(2. * np.pi * (x / d['grid']['Lx'] + y / d['grid']['Ly']))
    q[2] *= 1. + 0.01 * np.sin(2. * np.pi * (x / d['grid']['Lx'] - 2. * y / d['grid']['Ly']))
    if perturb_seed is not None:
        q[0] *= 1. + 2.2e-16 * np.random.default_rng(perturb_seed).standard_normal(q[0].shape)
    prob.q[...] = q
    prob.kinetic_energy_old = prob.kinetic_energy
    return prob


_ORACLE = {}


def oracle_run(case):
    """The oracle's run of a case, computed once per process and handed out read-only: dict with q0 (initial field), q, dt, ekin,
    mass, v_sound, tau_avg, viscosity (field or scalar), steps, stopped, and sens -- the response of q, per component and as a
    fraction of helpers.comp_err's scales, to one ulp of noise on the initial density (a second run of the oracle)."""
    if case.id not in _ORACLE:
        from oracle.problem import OracleProblem
        from helpers import comp_err
        runs = []
        for seed in (None, 11):
            p = make(OracleProblem, case, seed)
            q0 = p.q.copy()
            for _ in range(STEPS):
                p.update()
            runs.append((p, q0))
        (p, q0), (pert, _) = runs
        tau_avg = p.tau_avg.copy()      # as update() leaves it: the corrector stage's closure
        p.update_closures()             # (for the viscosity of the final state)
        out = dict(q0=q0, q=p.q.copy(), dt=p.dt, ekin=p.kinetic_energy, mass=p.mass, v_sound=p.v_sound, tau_avg=tau_avg,
                   viscosity=np.array(p.viscosity()), steps=p.step, stopped=p._stop, sens=comp_err(pert.q, p.q), prop=p.prop)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[case.id] = out
    return _ORACLE[case.id]


def _piezo_of(li, variant):
    """Barus and Roelands alternate over the pressure laws; Dukler and McAdams go with Bayada and with the power law (whose
    pressure never comes near zero, where McAdams' M = alpha rho_v / p has its pole)."""
    law = list(LAWS)[li]
    first = variant == 'piezo'
    if law in ('Bayada', 'PL'):
        return 'Dukler' if first else 'McAdams'
    return ('Barus', 'Roelands')[(li + (0 if first else 1)) % 2]


def _matrix():
    cases = []
    for li, law in enumerate(LAWS):
        for vi, variant in enumerate(VARIANTS):
            nx, ny = SHAPES[(li + vi) % 2]
            bc = ('pp', 'dd')[(li + vi // 2) % 2]
            piezo = _piezo_of(li, variant) if 'piezo' in variant else None
            cases.append(Case(f'{law}-{variant}-{nx}x{ny}-{bc}', law, variant, nx, ny, bc, piezo, 0))
    return cases


MATRIX = _matrix()
# TOPO 1 with dh/dy != 0: one light and one heavy law
LINE_HY = [Case('cubic-line-hy-37x40-pp', 'cubic', 'line-hy', 37, 40, 'pp', None, 0),
           Case('BWR-line-hy-14x130-dd', 'BWR', 'line-hy', 14, 130, 'dd', None, 0)]
# long marches: the four heavy laws (ring of 2 rows) and DH (GPF_K2_AHEAD_LINE), coefficients in the kernel and from the table
LONG = [Case(f'{law}-{variant}-long-{LONG_SHAPE[0]}x{LONG_SHAPE[1]}-{bc}', law, variant, *LONG_SHAPE, bc, None, LONG_CHUNKS)
        for law in ('PL', 'MT', 'BWR', 'Bayada', 'DH') for variant, bc in (('coef', 'pp'), ('table', 'dd'))]
CASES = MATRIX + LINE_HY + LONG
IDS = [c.id for c in CASES]
