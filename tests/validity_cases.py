"""The case table of tests/test_gpu_validity.py (the reductions that close a time step -- kinetic energy, max v^2, max c^2 and the
validity flags 1 NaN / 2 negative density / 4 imaginary sound speed -- with the maximum or the invalid cell planted at chosen
positions, on every step path) and of tests/test_validity_host.py (the table against its own claims, on the oracle alone).  Texts
and functions only.

Physics: tests/step_matrix_cases.py's (Lx = Ly = 1470, gap 12 .. 60, U 0.12, V 0.05, shear 2.15, MC_order 0), with a FIXED time
step of DT_FRACTION of the acoustic limit, so small that one step moves no planted quantity by more than a per cent of its distance
to the threshold it is meant to cross (the host test asserts it): whether the state after the step is valid, and where its maxima
sit, is then a property of the planted state and not of the dynamics.

Laws.  DH: light, a negative density stays finite in its closures (isolates flag 2), c^2 is a square (no flag 4).  BWR at T = 1: heavy,
stable at rho0 = 0.8, inside its spinodal (0.11 .. 0.58) at 0.5.  vdW at T = 100 (critical: 151): light; rho0 is moved to 3000 for
this table, just below the spinodal 4060 .. 18530, and the planted density is 4600.

Planted states.  Every state is the base state (uniform density, the smooth 1 % wave on both fluxes) with one interior cell changed
and the ghost cells refilled by the case's rules, so that a ghost cell is the rule's image of its interior cell before the step as
after it (the reference judges validity on the average of two ghosted arrays, the kernels on the rule's image of the average).
  spike     both fluxes doubled: (jx^2 + jy^2) / rho four times any other cell's
  below     D/N/N edges: a spike whose density is DELTA below the lowest adjacent Dirichlet target -- its ghost image is weaker
  above     D/N/N edges: a spike whose density is DELTA above the highest adjacent target -- a ghost cell alone holds the maximum
  spinodal  the density at which the law's sound speed is imaginary and its pressure finite
  image     D/N/N edges: a stable density whose Dirichlet image 2 target - rho is the spinodal density (a ghost cell alone)
  nan-rho, nan-jx, nan-jy, negative     one component NaN; the density - rho0
  ghost-negative   D/N/N edges: the density 2.2 targets, its image - 0.2 targets (a ghost cell alone)
  zero      rho = jx = jy = 0: no NaN and no negative density in the state; what the step makes of it the oracle decides
"""
import io
from collections import namedtuple

import numpy as np

import step_matrix_cases as M

DT_FRACTION = 2e-6
DELTA = 1e-3
ONE_WORKGROUP_CELLS = 1200          # small_grid_fits_lds: ghost cells included

PROPS = {'DH': M.LAWS['DH'].props, 'BWR': M.LAWS['BWR'].props,
         'vdW': 'EOS: vdW, rho0: 3000., M: 1000., T: 100., a: 1.355, b: 0.03201'}
RHO0 = {'DH': 877.7007, 'BWR': 0.8, 'vdW': 3000.}
HEAVY = {'DH': False, 'BWR': True, 'vdW': False}
SPINODAL = {'BWR': 0.5, 'vdW': 4600.}           # the planted density; a stable density beyond the far edge of the spinodal
SPINODAL_FAR = {'BWR': 0.05, 'vdW': 20000.}

VARIANTS = ['planes', 'slip', 'piezo', 'line', 'y-line', 'coef', 'table']
STEP2_SHAPES = [(14, 130, 0), (37, 40, 0), (230, 20, 2)]        # rows, columns, GPF_CHUNKS
SMALL_SHAPES = [(9, 20), (30, 1), (1, 30)]
MID_SHAPE = (37, 40)
PATHS = ('k_step2', 'k_small_steps', 'unfused', 'stagewise', 'split')
THINNING = ', thinning: {name: Carreau, mu_inf: 1.e-3, lam: 1.e-5, a: 2., N: 0.6}'

Case = namedtuple('Case', 'id law variant nx ny bc chunks path')

TEXT = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, Lx: 1470., Ly: 1470.{bc}}}
geometry: {{type: {gap}, hmin: 12., hmax: 60., U: 0.12, V: 0.05}}
numerics: {{CFL: 0.5, adaptive: 0, dt: {dt!r}, MC_order: 0, max_it: 1000000}}
properties: {{{law}, shear: 2.15, bulk: 0.{extra}}}
"""


def _case(law, variant, shape, bc, path):
    nx, ny = shape[:2]
    chunks = shape[2] if len(shape) > 2 else 0
    return Case(f'{path}-{law}-{variant}-{nx}x{ny}-{bc}', law, variant, nx, ny, bc, chunks, path)


def step2_cases(laws):
    """k_step2: the seven variants x three shapes x the given laws; the edges alternate down the table (each variant and each
    shape meets both kinds)."""
    out = []
    for li, law in enumerate(laws):
        for vi, variant in enumerate(VARIANTS):
            for si, shape in enumerate(STEP2_SHAPES):
                out.append(_case(law, variant, shape, ('pp', 'dd')[(li + vi + si) % 2], 'k_step2'))
    return out


def other_cases(laws):
    """k_small_steps at its three shapes, the two pipelines and the split edge form at 37 x 40; D/N/N edges and periodic ones."""
    out = []
    for law in laws:
        for si, shape in enumerate(SMALL_SHAPES):
            out += [_case(law, 'planes', shape, bc, 'k_small_steps') for bc in (('pp', 'dd') if si == 0 else (('dd', 'pp')[si - 1],))]
        for pi, path in enumerate(('unfused', 'stagewise', 'split')):
            out.append(_case(law, 'planes', MID_SHAPE, ('dd', 'pp')[pi % 2], path))
    return out


MAX_CASES = step2_cases(('DH', 'BWR')) + other_cases(('DH', 'BWR'))
SOUND_CASES = step2_cases(('vdW', 'BWR')) + other_cases(('vdW', 'BWR'))
INVALID_CASES = step2_cases(('DH',)) + other_cases(('DH',))
ENSEMBLE_SHAPES = {'lds': (9, 20), 'workspace': MID_SHAPE}


_PROPS = {}


def props_of(law):
    if law not in _PROPS:
        import yaml
        from oracle.config import sanitize_properties
        _PROPS[law] = sanitize_properties(yaml.full_load('{' + PROPS[law] + ', shear: 2.15, bulk: 0.}'))
    return _PROPS[law]


def sound_speed(law, rho):
    from oracle import closures as cl
    with np.errstate(invalid='ignore'):
        return cl.eos_sound_speed(np.asarray(rho, float), props_of(law))


def pressure(law, rho):
    from oracle import closures as cl
    return cl.eos_pressure(np.asarray(rho, float), props_of(law))


def spinodal_edge(law, inside, outside):
    """The density between `inside` (imaginary sound speed) and `outside` (real) at which dp/drho changes sign, by bisection."""
    a, b = float(inside), float(outside)
    assert np.isnan(sound_speed(law, a)) and not np.isnan(sound_speed(law, b))
    for _ in range(60):
        m = 0.5 * (a + b)
        a, b = (m, b) if np.isnan(sound_speed(law, m)) else (a, m)
    return 0.5 * (a + b)


def dt_of(case):
    """DT_FRACTION of min(dx, dy) / c(rho0)."""
    return float(DT_FRACTION * min(1470. / case.nx, 1470. / case.ny) / sound_speed(case.law, RHO0[case.law]))


def targets_of(case):
    """{side: Dirichlet density} of a D/N/N case (step_matrix_cases.DD_FRACTIONS of rho0), None for periodic edges."""
    if case.bc != 'dd':
        return None
    return dict(zip(('xE', 'xW', 'yS', 'yN'), (f * RHO0[case.law] for f in M.DD_FRACTIONS)))


def piezo_text(case):
    """Barus, a factor of 1.5 over the largest pressure any density of this table gives the law."""
    rho0, t = RHO0[case.law], max(M.DD_FRACTIONS)
    rhos = [rho0, -rho0, 0., 2.2 * t * rho0, -0.2 * t * rho0] + ([SPINODAL[case.law]] if case.law in SPINODAL else [])
    return f', piezo: {{name: Barus, aB: {float(np.log(1.5) / np.abs(pressure(case.law, rhos)).max())!r}}}'


def case_text(case):
    gap = {'planes': 'asperity, num: 1', 'slip': 'asperity, num: 1', 'piezo': 'asperity, num: 1', 'line': 'parabolic', 'coef': 'parabolic',
           'table': 'inclined', 'y-line': 'parabolic'}[case.variant]
    t = targets_of(case)
    bc = M.DD.format(*(repr(t[s]) for s in ('xE', 'xW', 'yS', 'yN'))) if t else ''
    extra = (piezo_text(case) if case.variant == 'piezo' else '') + (THINNING if case.path == 'stagewise' else '')
    return TEXT.format(nx=case.nx, ny=case.ny, bc=bc, gap=gap, dt=dt_of(case), law=PROPS[case.law], extra=extra)


def env_of(case):
    """Environment of the GPU run, in force from before the handle is created to after its last step."""
    env = M.env_of(case)
    if case.path == 'split':            # read by gpf_create, and set means on: the GPU test clears it before every test
        env['GPF_STEP_UNFUSED_EDGES'] = '1'
    return env


def expected_kernel(case, step):
    """gpf_step_variant's answer for the step taken from step index `step` (MC_order 0: D = +1 from an even index)."""
    has_ls, piezo, topo = M.EXPECTED[case.variant]
    return (M.EOS_ID[case.law], has_ls, piezo, 1 if step % 2 == 0 else -1, topo)


def fill_ghosts(q, case):
    """The ghost cells of q by the case's rules, in place: the x edges over all columns, then the y edges over all rows (problem.py:
    676-768; the low-x ghost takes xW's target and the low-y ghost yN's, as oracle/problem.py restates it)."""
    t = targets_of(case)
    if t is None:
        q[:, 0, :], q[:, -1, :] = q[:, -2, :].copy(), q[:, 1, :].copy()
        q[:, :, 0], q[:, :, -1] = q[:, :, -2].copy(), q[:, :, 1].copy()
        return q
    q[0, 0, :], q[0, -1, :] = (t['xW'] - 0.5 * q[0, 1, :]) / 0.5, (t['xE'] - 0.5 * q[0, -2, :]) / 0.5
    q[1:, 0, :], q[1:, -1, :] = q[1:, 1, :], q[1:, -2, :]
    q[0, :, 0], q[0, :, -1] = (t['yN'] - 0.5 * q[0, :, 1]) / 0.5, (t['yS'] - 0.5 * q[0, :, -2]) / 0.5
    q[1:, :, 0], q[1:, :, -1] = q[1:, :, 1], q[1:, :, -2]
    return q


def images_of(case, pos):
    """The cells that hold the rule's image of interior cell pos = (ix, iy), itself included: up to three ghost cells."""
    ix, iy = pos
    xs, ys = [ix], [iy]
    if case.bc == 'pp':
        xs += [case.nx + 1] * (ix == 1) + [0] * (ix == case.nx)
        ys += [case.ny + 1] * (iy == 1) + [0] * (iy == case.ny)
    else:
        xs += [0] * (ix == 1) + [case.nx + 1] * (ix == case.nx)
        ys += [0] * (iy == 1) + [case.ny + 1] * (iy == case.ny)
    return sorted({(a, b) for a in xs for b in ys})


def adjacent_targets(case, pos):
    """The Dirichlet densities behind the ghost cells next to pos (the side-swapped ones the rules really use)."""
    t, (ix, iy) = targets_of(case), pos
    return ([t['xW']] * (ix == 1) + [t['xE']] * (ix == case.nx) + [t['yN']] * (iy == 1) + [t['yS']] * (iy == case.ny)) if t else []


def interior(case):
    return [(ix, iy) for ix in range(1, case.nx + 1) for iy in range(1, case.ny + 1)]


def edge_cells(case):
    return [p for p in interior(case) if p[0] in (1, case.nx) or p[1] in (1, case.ny)]


def make(cls, case):
    """Problem or OracleProblem of a case after _pre_run(), holding the base state."""
    from oracle.topography import midpoint_grid
    reader = None
    if cls.__module__.startswith('gapflow_amd'):
        from gapflow_amd.io import read_yaml_input as reader
    else:
        from oracle.config import read_yaml_input as reader
    with io.StringIO(case_text(case)) as f:
        d = reader(f)
    extra = M.slip_field(case, d['grid']) if 'slip' in case.variant else None
    prob = cls(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'], extra_field=extra)
    planes = M.planes_of(case, d['grid'])
    if planes is not None:
        if hasattr(prob, '_upload_topo'):
            prob.topo.full[:3] = planes
            prob._upload_topo()
        else:
            prob.topo[:3] = planes
    prob._pre_run()
    x, y = midpoint_grid(d['grid'])
    q = np.array(prob.q)
    q[1] *= 1. + 0.01 * np.cos(2. * np.pi * (x / d['grid']['Lx'] + y / d['grid']['Ly']))
    q[2] *= 1. + 0.01 * np.sin(2. * np.pi * (x / d['grid']['Lx'] - 2. * y / d['grid']['Ly']))
    prob.q[...] = fill_ghosts(q, case)
    prob.kinetic_energy_old = prob.kinetic_energy
    return prob


_BASE = {}


def base_state(case):
    """The base state of a case (from the oracle's constructor), computed once and handed out read-only."""
    key = case.id.split('-', 1)[1]
    if key not in _BASE:
        from oracle.problem import OracleProblem
        q = make(OracleProblem, case).q.copy()
        q.setflags(write=False)
        _BASE[key] = q
    return _BASE[key]


KINDS_MAX = ('spike', 'below', 'above')
KINDS_SOUND = ('spinodal', 'image')
KINDS_INVALID = ('nan-rho', 'nan-jx', 'nan-jy', 'negative', 'ghost-negative')
NEEDS_EDGE = ('below', 'above', 'image', 'ghost-negative')


def plant(case, kind, pos, q=None):
    """The base state (or q) with `kind` planted in interior cell pos, ghost cells refilled.  Returns a new array."""
    q = np.array(base_state(case) if q is None else q)
    ix, iy = pos
    assert 1 <= ix <= case.nx and 1 <= iy <= case.ny
    rho0 = RHO0[case.law]
    if kind in NEEDS_EDGE:
        t = adjacent_targets(case, pos)
        assert t, f'{kind} needs a cell next to a Dirichlet edge'
    if kind in KINDS_MAX:
        q[1:, ix, iy] *= 2.
        if kind == 'below':
            q[0, ix, iy] = min(t) * (1. - DELTA)
        elif kind == 'above':
            q[0, ix, iy] = max(t) * (1. + DELTA)
    elif kind == 'spinodal':
        q[0, ix, iy] = SPINODAL[case.law]
    elif kind == 'image':
        q[0, ix, iy] = 2. * t[0] - SPINODAL[case.law]
    elif kind.startswith('nan-'):
        q[('rho', 'jx', 'jy').index(kind[4:]), ix, iy] = np.nan
    elif kind == 'negative':
        q[0, ix, iy] = -rho0
    elif kind == 'ghost-negative':
        q[0, ix, iy] = 2.2 * max(t)
    elif kind == 'zero':
        q[:, ix, iy] = 0.
    else:
        raise ValueError(kind)
    return fill_ghosts(q, case)


def invalid_positions(case):
    """Part 3's interior cells that take every kind, ghosted indices: the four corners, the middle of each edge row and column, the
    middle cell, and
      14 x 130   columns 126 | 127 (the seam of the two strips) and 130 (the last of the four-column strip)
      230 x 20   rows 115 | 116 (the chunks' seam with GPF_CHUNKS=2)."""
    nx, ny = case.nx, case.ny
    mx, my = (nx + 1) // 2, (ny + 1) // 2
    cells = [(1, 1), (1, ny), (nx, 1), (nx, ny), (1, my), (nx, my), (mx, 1), (mx, ny), (mx, my)]
    if (nx, ny) == (14, 130):
        cells += [(mx, 126), (mx, 127), (mx, 130)]
    if (nx, ny) == (230, 20):
        cells += [(115, my), (116, my)]
    return sorted(set(cells))


ROW_SWEEP_KINDS = ('nan-jy', 'negative')


def row_sweep(case):
    """Every row at the middle column (14 x 130: at columns 2 and 128, one in each strip whichever way the strips are counted), for
    ROW_SWEEP_KINDS: whatever the plan, the first and the last row of every row chunk and a row of every wave of every block, the
    last one included."""
    cols = [2, 128] if (case.nx, case.ny) == (14, 130) else [(case.ny + 1) // 2]
    return [(ix, iy) for iy in cols for ix in range(1, case.nx + 1)]


STRIP_COLUMNS = 126         # output columns of one wavefront of k_step2


def wave_of(case, nchunks, pos, D):
    """(block, wave) of k_step2 that writes interior cell pos when the predictor runs in direction D and the plan holds nchunks row
    chunks per strip: a wave marches rows 1 + c Nx / nchunks .. (c + 1) Nx / nchunks of strip s, counted from the far end when D < 0;
    wave c nstrips + s; four waves to a block (step2_kernel.hip)."""
    n, m = (pos if D > 0 else (case.nx + 1 - pos[0], case.ny + 1 - pos[1]))
    chunk = next(c for c in range(nchunks) if 1 + c * case.nx // nchunks <= n <= (c + 1) * case.nx // nchunks)
    nstrips = -(-case.ny // STRIP_COLUMNS)
    w = chunk * nstrips + (m - 1) // STRIP_COLUMNS
    return w // 4, w


def far_pair(case):
    """Two interior cells as far apart as the shape allows -- the first and the last wave of any plan -- for a NaN and a negative
    density at once."""
    return (1, 1), (case.nx, case.ny)


def slab_jobs(case, layouts):
    """Part 3 and 4 on x-slabs; layouts: (lo, hi) first and last row of every rank.  In each rank in turn a cell on a seam row (a
    row its neighbour reads) and one away from it, for nan-jy / negative / zero; a ghost-only negative density on each x edge and
    on a y edge of the middle rank; a NaN in the first rank with a negative density in the last."""
    my = (case.ny + 1) // 2
    jobs = []
    for r, (lo, hi) in enumerate(layouts):
        seam = hi if r + 1 < len(layouts) else lo
        for pos in ((seam, my), ((lo + hi) // 2, 3)):
            jobs += [(f'rank {r}: {kind} at {pos}', plant(case, kind, pos), [pos]) for kind in ('nan-jy', 'negative', 'zero')]
    if case.bc == 'dd':
        mid = layouts[len(layouts) // 2]
        for pos in ((1, my), (case.nx, my), ((mid[0] + mid[1]) // 2, 1)):
            jobs.append((f'ghost-negative at {pos}', plant(case, 'ghost-negative', pos), [pos]))
    a, b = far_pair(case)
    jobs.append((f'nan-jy at {a} and negative at {b}', plant(case, 'negative', b, plant(case, 'nan-jy', a)), [a, b]))
    return jobs


SLAB_RANKS = 3
SLAB_CASE = _case('DH', 'planes', MID_SHAPE, 'dd', 'slabs')


def trial_step(p):
    """OracleProblem.update() up to the average, without the decision: the state the validity is judged on (problem.py:563)."""
    mc = p.numerics['MC_order']
    switch = (p.step % 2 == 0) * 2 - 1 if mc == 0 else mc
    q0 = p.q.copy()
    with np.errstate(all='ignore'):
        for i, d in enumerate([[-1, 1], [1, -1]][(switch + 1) // 2]):
            p.stage(d, p.dt, predictor=(i == 0), compute_var=False)
    out = (p.q + q0) / 2.0
    p.q[...] = q0
    return out


def oracle_outcome(case, q, steps_before=0):
    """What OracleProblem.update() makes of state q: dict with stopped, step (after), invalid (1: a NaN in the judged state, 2:
    a negative density only, 0: committed), q (after), pressure (of update_closures(False, True) behind a refused step, else None),
    ekin, v_max, v_sound of the committed state."""
    from oracle.problem import OracleProblem
    p = make(OracleProblem, case)
    p.step = steps_before
    p.q[...] = q
    judged = trial_step(p)
    with np.errstate(all='ignore'):
        p.update()
        out = dict(stopped=p._stop, step=p.step, q=p.q.copy(), judged=judged,
                   invalid=0 if not p._stop else (1 if np.isnan(judged).any() else 2), pressure=p.pressure.copy() if p._stop else None)
        if not p._stop:
            out.update(ekin=p.kinetic_energy, v_max=p.v_max, v_sound=p.v_sound)
    return out


def reference_scalars(q, law):
    """oracle/problem.py's kinetic_energy, v_max, v_sound on a ghosted array, NumPy fp64; and the argmax of v."""
    q = np.asarray(q, float)
    v = (q[1]**2 + q[2]**2) / q[0]
    return np.sum(v / 2.), np.sqrt(v).max(), sound_speed(law, q[0]).max(), np.unravel_index(np.argmax(v), v.shape)
