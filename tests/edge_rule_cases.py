"""The case table of tests/test_gpu_edge_rules.py (every ghost-cell rule triple on every step path, against the oracle) and of
tests/test_edge_rules_host.py (the table against its own claims, on the oracle alone).  Texts and functions only.

A non-periodic edge carries one rule per component of (rho, jx, jy) -- D: ghost = 2 target - adjacent, N: ghost = adjacent -- and
one target per edge; both edges of an axis declare the same triple (Problem._edge_rules refuses anything else), or the axis is
periodic.  TRIPLES: the eight D/N triples and PPP; a pair is (x triple, y triple): 81 of them.

Targets: all four unequal, so that a value taken from the wrong edge or from the swapped side shows in every Dirichlet component.
A triple whose density is Dirichlet takes density-like targets, one whose density is not takes flux-like ones; for the flux of
a `DDx` triple (a density-like target on jx ~ 88) that is violent on purpose, and the host test shows that six steps survive it.
An edge without any D has no target at all: the reference itself raises KeyError there (problem.py:739-753 read the value before
the mask), so such an edge is an extension of gapflow_amd, with the meaning "copy the adjacent cell".

Physics: test_gpu_ragged.py's (Dowson-Higginson with C1 3.5e9, shear 0.0794, bulk 0.02, one asperity, U 0.2, V 0.1); the sweep
order rotates over MC_order 1 / -1 / 0 with the pair's index.  The initial state carries the smooth 1 % wave of
step_matrix_cases.make on both fluxes, so that no ghost value coincides with its neighbour's.

Shapes (rows x columns), the smallest at which each path can still go wrong:
  14 x 130   k_step2: two strips, the second holding 4 columns, the ghost column and its idle lanes
  37 x 40    k_step2: one partial strip, rows that do not divide into the chunks; k_mid_ensemble when forced; the split form,
             the reference-ordered pipeline and the stage-wise pipeline (shear thinning)
  9 x 20, 30 x 1, 1 x 30   k_small_steps (one workgroup); the 1-D shapes with the other axis periodic
"""
import io

import numpy as np

STEPS = 6
TRIPLES = ['DDD', 'DDN', 'DND', 'DNN', 'NDD', 'NDN', 'NND', 'NNN', 'PPP']
DN_TRIPLES = TRIPLES[:8]
PAIRS = [(x, y) for x in TRIPLES for y in TRIPLES]
MC_ORDERS = (1, -1, 0)

# (xE, xW) and (yS, yN), by whether the triple's density is Dirichlet
TARGETS = {('x', True): (877.7007, 876.), ('x', False): (87.77, 60.),
           ('y', True): (878.2007, 876.25), ('y', False): (88.27, 60.25)}

STEP2_SHAPES = [(14, 130), (37, 40)]
SMALL_SHAPE, ROW_SHAPE, COLUMN_SHAPE = (9, 20), (30, 1), (1, 30)
MID_SHAPE = (37, 40)
# the diagonal of the eight D/N triples and eight pairs whose x and y rules differ per component
SIXTEEN = [(t, t) for t in DN_TRIPLES] + [('NDD', 'DNN'), ('DNN', 'NDD'), ('NNN', 'DDD'), ('DDD', 'NNN'), ('PPP', 'NDN'), ('NDN', 'PPP'),
                                          ('DND', 'NND'), ('NND', 'DND')]
# slabs (cut along x): a non-periodic x triple with a D on a flux, and a y triple different from it
SLAB_PAIRS = [('NDD', 'DNN'), ('DND', 'NND'), ('NND', 'DND'), ('NDN', 'PPP')]
SLAB_SHAPE = (37, 40)
# shear thinning: the Carreau case of test_gpu_extras.test_shear_thinning_steps_match_oracle
THINNING = ', thinning: {name: Carreau, mu_inf: 1.e-3, lam: 1.e-5, a: 2., N: 0.6}'

TEXT = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, {size}{bc}}}
geometry: {{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.2, V: 0.1}}
numerics: {{CFL: 0.4, adaptive: 1, dt: 2.e-10, MC_order: {mc}, max_it: 100}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0.02, rho0: 877.7007, C1: 3.5e9{extra}}}
"""


def pair_id(pair):
    return f'{pair[0]}x{pair[1]}'


def mc_order_of(pair):
    return MC_ORDERS[PAIRS.index(tuple(pair)) % 3]


def row_pairs():
    """30 x 1: the x triples, y periodic."""
    return [(t, 'PPP') for t in TRIPLES]


def column_pairs():
    """1 x 30: the y triples, x periodic."""
    return [('PPP', t) for t in TRIPLES]


def targets_of(pair):
    """{side: Dirichlet target} of the sides whose triple has a D."""
    out = {}
    for axis, triple, sides in (('x', pair[0], ('xE', 'xW')), ('y', pair[1], ('yS', 'yN'))):
        if 'D' in triple:
            out.update(zip(sides, TARGETS[axis, triple[0] == 'D']))
    return out


def rules_of(pair):
    """{side: triple} for reference_ghosts."""
    return {'xE': pair[0], 'xW': pair[0], 'yS': pair[1], 'yN': pair[1]}


def case_text(pair, shape, targets=None, mc=None, thinning=False, lengths=None):
    """targets: {side: value} in place of targets_of(pair) (the host test swaps them); mc: in place of the pair's own; lengths:
    (Lx, Ly) in place of the cell size 2e-5 x 2.5e-5 (two grids of one domain, for init_from)."""
    targets = targets_of(pair) if targets is None else targets
    bc = ''
    for triple, sides in ((pair[0], ('xE', 'xW')), (pair[1], ('yS', 'yN'))):
        if triple == 'PPP':
            continue
        for s in sides:
            bc += f', {s}: {list(triple)!r}'
            if 'D' in triple:
                bc += f', {s}_D: {targets[s]!r}'
    size = 'dx: 2.e-5, dy: 2.5e-5' if lengths is None else f'Lx: {lengths[0]!r}, Ly: {lengths[1]!r}'
    return TEXT.format(nx=shape[0], ny=shape[1], size=size, bc=bc, mc=mc_order_of(pair) if mc is None else mc, extra=THINNING if thinning else '')


def field_err(a, b):
    """max |a - b| per component, as a fraction of that component's own scale max |b| (test_gpu_ragged.run_case)."""
    return np.array([np.abs(x - y).max() / (np.abs(y).max() or 1.) for x, y in zip(np.asarray(a, float), np.asarray(b, float))])


def wave(q, grid):
    """step_matrix_cases.make's initial state: the smooth 1 % wave on both fluxes, ghost cells included."""
    from oracle.topography import midpoint_grid
    x, y = midpoint_grid(grid)
    q = q.copy()
    q[1] *= 1. + 0.01 * np.cos(2. * np.pi * (x / grid['Lx'] + y / grid['Ly']))
    q[2] *= 1. + 0.01 * np.sin(2. * np.pi * (x / grid['Lx'] - 2. * y / grid['Ly']))
    return q


def make(cls, pair, shape, perturb_seed=None, **text_args):
    """Problem or OracleProblem of (pair, shape) after _pre_run(), on the wave.  perturb_seed: one ulp of relative noise on the
    initial density."""
    if cls.__module__.startswith('gapflow_amd'):
        from gapflow_amd.io import read_yaml_input as reader
    else:
        from oracle.config import read_yaml_input as reader
    with io.StringIO(case_text(pair, shape, **text_args)) as f:
        d = reader(f)
    prob = cls(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'])
    prob._pre_run()
    q = wave(prob.q, d['grid'])
    if perturb_seed is not None:
        q[0] *= 1. + 2.2e-16 * np.random.default_rng(perturb_seed).standard_normal(q[0].shape)
    prob.q[...] = q
    prob.kinetic_energy_old = prob.kinetic_energy
    return prob


def oracle_steps(pair, shape, perturb_seed=None, **text_args):
    from oracle.problem import OracleProblem
    p = make(OracleProblem, pair, shape, perturb_seed, **text_args)
    q0 = p.q.copy()
    for _ in range(STEPS):
        p.update()
    return p, q0


_ORACLE = {}


def oracle_run(pair, shape, thinning=False):
    """The oracle's six steps of (pair, shape), computed once per process and handed out read-only: dict with q0 (initial field),
    q, dt, ekin, mass, steps, stopped, and sens -- the response of q, per component and as a fraction of its scale, to one ulp of
    noise on the initial density (a second run of the oracle)."""
    key = (tuple(pair), tuple(shape), thinning)
    if key not in _ORACLE:
        p, q0 = oracle_steps(pair, shape, thinning=thinning)
        pert, _ = oracle_steps(pair, shape, perturb_seed=11, thinning=thinning)
        out = dict(q0=q0, q=p.q.copy(), dt=p.dt, ekin=p.kinetic_energy, mass=p.mass, steps=p.step, stopped=p._stop,
                   sens=field_err(pert.q, p.q))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def reference_ghosts(q, rules, values):
    """problem.py:676-768 for one ghosted array q (ncomp, Nx+2, Ny+2), cell by cell: returns a copy of q with its ghost cells
    filled.  rules: {side: triple of 'D' / 'N' / 'P' per component}, values: {side: Dirichlet target} (only sides with a D).

    The x edges over ALL columns (ghost columns included), then the y edges over all rows, so that a corner is
    rule_y(rule_x(.)).  Whether an edge is periodic and which components a rule is assigned to come from one side's triple, the
    rule's own components and its target from the other (low x: assigned by xE, data of xW; high x: xW / xE; low y: yS / yN;
    high y: yN / yS -- the low-y ghost takes the yN value and the high-y ghost the yS value).  The reference pairs the k-th
    assigned component with the k-th data component; with equal triples on both sides of an axis, which is all a problem
    accepts, that is component by component."""
    q = np.array(q, dtype=float)
    ncomp, nx, ny = q.shape[0], q.shape[1] - 2, q.shape[2] - 2

    def ghost(rule, side, adjacent):
        if rule == 'D':
            return (values[side] - 0.5 * adjacent) / 0.5
        return (0.5 * adjacent) / 0.5

    for assign, data, ghost_row, adjacent_row, partner_row in (('xE', 'xW', 0, 1, nx), ('xW', 'xE', nx + 1, nx, 1)):
        assert sorted(rules[assign]) == sorted(rules[data]) and len(rules[assign]) == ncomp
        for c in range(ncomp):
            for iy in range(ny + 2):
                if all(r == 'P' for r in rules[assign]):
                    q[c, ghost_row, iy] = q[c, partner_row, iy]
                else:
                    assert rules[assign][c] == rules[data][c] != 'P'
                    q[c, ghost_row, iy] = ghost(rules[data][c], data, q[c, adjacent_row, iy])
    for assign, data, ghost_col, adjacent_col, partner_col in (('yS', 'yN', 0, 1, ny), ('yN', 'yS', ny + 1, ny, 1)):
        assert sorted(rules[assign]) == sorted(rules[data]) and len(rules[assign]) == ncomp
        for c in range(ncomp):
            for ix in range(nx + 2):
                if all(r == 'P' for r in rules[assign]):
                    q[c, ix, ghost_col] = q[c, ix, partner_col]
                else:
                    assert rules[assign][c] == rules[data][c] != 'P'
                    q[c, ix, ghost_col] = ghost(rules[data][c], data, q[c, ix, adjacent_col])
    return q
