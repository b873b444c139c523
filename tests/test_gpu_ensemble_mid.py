"""Ensembles, workspace tier (k_mid_ensemble, csrc/mid_kernel.hip): 2-D members of 1201 .. 16384 cells, ghost cells included, one
workgroup each, their planes in a workspace in device memory.

Yardsticks.  (1) The reference's recorded results: every 2-D fixture under tests/golden/ at every snapshot, at the tolerances of
test_gpu_parity.test_fused_step_matches_golden (helpers.field_tol / history_tol, the same rule for ILL_CONDITIONED_CASES) -- and
all 16 fixtures with the tier forced, which brings the seven equations of state and the wave start.  (2) Bit-for-bit equality
where the same kernel runs the same member: whoever else is in the ensemble, in whatever order, however the steps are split into
calls, with more members than the chip has compute units.  (3) The LDS tier on the same problem, at the bounds
test_gpu_extras.test_small_grid_kernel_equals_launch_per_kernel_path sets for two evaluation orders of that problem.  (4) The
oracle at the largest shape, 126 x 126.
Shapes: the fixtures' own (1764 .. 5984 cells: 4 .. 12 cells per thread, long and narrow seams included), 40 x 40 for the 260
members, 126 x 126 (32 cells per thread, the limit) and 127 x 126 (refused)."""
import ctypes as C

import numpy as np
import pytest

from helpers import STEP_CASES, load_case, comp_err, field_tol, history_tol, FIELD_RTOL, ILL_CONDITIONED_CASES
from test_gpu_ensemble import journal, build, quiet, mirror, assert_bitwise, assert_same_state
from test_gpu_parity import make_problem, check_history

pytestmark = pytest.mark.gpu

TWO_D = [n for n in STEP_CASES if min(load_case(n)[0]['q_init'].shape[1:]) > 3]


def state_of(p):
    q = p.q.copy()
    q.flags.writeable = False
    return dict(q=q, mirror=mirror(p), history={k: list(v) for k, v in p.history.items()})


def assert_same_member(p, ref, what):
    """q, the scalars and history, bit for bit (test_gpu_ensemble.assert_same_state and the history on top)."""
    assert_same_state(p, ref, what)
    assert p.history.keys() == ref['history'].keys()
    for k in ref['history']:
        assert_bitwise(p.history[k], ref['history'][k], f"{what}: history['{k}']")


def check_goldens(names, tier):
    """One ensemble of the named fixtures; each member stepped to its own snapshots with per-member counts; at each snapshot the
    checks of test_fused_step_matches_golden."""
    from gapflow_amd import Ensemble
    made = [make_problem(n) for n in names]
    ps = [m[0] for m in made]
    for name, (p, fx, meta) in zip(names, made):
        np.testing.assert_allclose(p.topo.full, fx['topo'], rtol=1e-14, atol=0)
        assert comp_err(p.q, fx['q_init']).max() == 0.0
    ens = Ensemble(ps, tier=tier)
    assert ens.tiers == ['workspace'] * len(ps)
    for s in sorted({s for _, _, meta in made for s in meta['snaps']}):
        due = [s in meta['snaps'] for _, _, meta in made]
        quiet(ens.step, [s - p.step if d else 0 for p, d in zip(ps, due)])
        for name, (p, fx, meta), d in zip(names, made, due):
            if not d:
                continue
            tol = field_tol(fx, s)
            if name not in ILL_CONDITIONED_CASES:       # every component of every snapshot is a real check
                assert (tol <= 1e-8).all(), f'{name}: snapshot {s} is conditioned to {tol} only'
            err = comp_err(p.q, fx[f'q_{s}'])
            print(f'[{name}] step {s}: err {err} tol {tol}')
            assert (err <= tol).all(), f'{name}: q at step {s}: err {err} tol {tol}'
            drho = np.abs(p.q[0] - fx[f'q_{s}'][0]).max()
            dp = np.abs(p.pressure.pressure - fx[f'p_{s}']).max()
            assert dp <= 1e-9 * np.abs(fx[f'p_{s}']).max() + 2.0 * p.pressure.v_sound**2 * drho, f'{name}: p at step {s}'
            check_history(fx['history'][s - 1], p, history_tol(fx))


def test_goldens_automatic_tier(hiplib):
    """1. Every 2-D fixture in one ensemble: all get the workspace tier by themselves."""
    assert len(TWO_D) >= 7 and 'journal2d_periodic50' in TWO_D and 'seam2d_asperity' in TWO_D
    check_goldens(TWO_D, 'auto')


def test_goldens_forced_workspace(hiplib):
    """2. All fixtures with tier='workspace': the 1-D ones (one cell per thread or less) bring all seven EOS and the wave start."""
    assert len(STEP_CASES) >= 16
    check_goldens(STEP_CASES, 'workspace')


_TWENTY = {}


def twenty_alone(name):
    """Fixture `name` after 20 steps as an ensemble of one: computed once, shared, left unchanged."""
    from gapflow_amd import Ensemble
    if name not in _TWENTY:
        p = make_problem(name)[0]
        quiet(Ensemble([p]).step, 20)
        _TWENTY[name] = state_of(p)
    return _TWENTY[name]


def test_independent_of_composition_and_of_batching(hiplib):
    """3a. A member in the ensemble of all 2-D fixtures, stepped 7 + 13; in the reversed ensemble, stepped 20; in an ensemble of
    one, stepped 20: the same bits."""
    from gapflow_amd import Ensemble
    fwd = [make_problem(n)[0] for n in TWO_D]
    ens = Ensemble(fwd)
    quiet(ens.step, 7)
    quiet(ens.step, 13)
    rev = [make_problem(n)[0] for n in reversed(TWO_D)]
    quiet(Ensemble(rev).step, 20)
    for k, name in enumerate(TWO_D):
        ref = twenty_alone(name)
        assert ref['mirror'][0] == 20
        assert_same_member(fwd[k], ref, f"{name}, step(7) + step(13) among {len(TWO_D)}")
        assert_same_member(rev[len(TWO_D) - 1 - k], ref, f"{name}, reversed order")


def test_more_members_than_compute_units(hiplib):
    """3b. 260 members of the 40 x 40 journal, 13 eccentricities x 20 copies, 10 steps: workgroups that follow one another on a
    CU, each on its own workspace.  Copies are equal bit for bit, and equal to their ensemble of one."""
    from gapflow_amd import Ensemble
    eps = [0.3 + 0.05 * k for k in range(13)]
    texts = [journal(40, ny=40, eps=e, U=10.) for e in eps]
    ps = [build(texts[m % 13]) for m in range(260)]
    ens = Ensemble(ps)
    assert set(ens.tiers) == {'workspace'}
    quiet(ens.step, 10)
    for k, t in enumerate(texts):
        one = build(t)
        quiet(Ensemble([one]).step, 10)
        ref = state_of(one)
        assert ref['mirror'][0] == 10
        for m in range(k, 260, 13):
            assert_same_member(ps[m], ref, f"member {m} (eps {eps[k]:.2f})")
    assert not np.array_equal(ps[0].q, ps[1].q)             # the eccentricities do differ


def test_mixed_tiers(hiplib):
    """4. A 1-D member, a 50 x 50 member and a 40 x 40 member with a slip-length field: three launch groups over two tiers; the
    LDS member is bit for bit its solo run, the others their ensembles of one."""
    from gapflow_amd import Ensemble
    cases = [(journal(100, mc=1), False), (journal(50, ny=50, eps=0.5, U=10.), False), (journal(40, ny=40, eps=0.6, U=10.), True)]
    ps = [build(t, s) for t, s in cases]
    ens = Ensemble(ps)
    assert ens.tiers == ['lds', 'workspace', 'workspace']
    info = [(C.c_int32(-1), C.c_int64(-1)) for _ in ps]
    for m, (tier, nbytes) in enumerate(info):
        assert hiplib.gpf_ensemble_member_info(ens._e, m, C.byref(tier), C.byref(nbytes)) == 0
    from gapflow_amd.ensemble import workspace_bytes
    assert [(t.value, b.value) for t, b in info] == [(0, 0), (1, workspace_bytes(50, 50)), (1, workspace_bytes(40, 40))]
    quiet(ens.step, 21)
    solo = build(*cases[0])
    quiet(solo._advance, 21, honor_stop=False)
    assert_same_state(ps[0], dict(q=solo.q, mirror=mirror(solo)), 'the LDS member against its solo run')
    for m in (1, 2):
        one = build(*cases[m])
        quiet(Ensemble([one]).step, 21)
        assert_same_member(ps[m], state_of(one), f"member {m} against its ensemble of one")
        assert np.isfinite(ps[m].q).all() and ps[m].step == 21


ASPERITY_33x17 = """
options: {silent: True}
grid: {Nx: 33, Ny: 17, Lx: 0.01, Ly: 0.005, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 876.,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.1}
numerics: {CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1.e-14, max_it: 100000}
properties: {EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007, piezo: {name: Barus, aB: 2.e-8}}
"""


def test_same_problem_in_both_tiers(hiplib):
    """5. The 33 x 17 asperity problem of test_small_grid_kernel_equals_launch_per_kernel_path, 37 + 40 steps, once per tier, at
    that test's bounds for two evaluation orders of this problem.  (Whether it came out bit for bit is printed)"""
    from gapflow_amd import Ensemble, Problem
    out = {}
    for tier in ('auto', 'workspace'):
        p = quiet(Problem.from_string, ASPERITY_33x17)
        quiet(p._pre_run)
        ens = Ensemble([p], tier=tier)
        assert ens.tiers == [{'auto': 'lds', 'workspace': 'workspace'}[tier]]
        quiet(ens.step, 37)
        quiet(ens.step, 40)
        out[tier] = p
    a, b = out['auto'], out['workspace']
    assert a.step == b.step == 77
    same = np.array_equal(a.q, b.q) and a.dt == b.dt and a.simtime == b.simtime and a.kinetic_energy == b.kinetic_energy
    print('\n[33 x 17, 77 steps] LDS tier and workspace tier: ' + ('bit for bit' if same else 'max |dq| / scale = ' +
          ', '.join(f'{np.abs(a.q[c] - b.q[c]).max() / np.abs(a.q[c]).max():.1e}' for c in range(3))))
    for c in range(3):
        assert np.abs(a.q[c] - b.q[c]).max() <= 1e-10 * np.abs(a.q[c]).max(), c
    np.testing.assert_allclose(b.dt, a.dt, rtol=1e-13)
    np.testing.assert_allclose(b.simtime, a.simtime, rtol=1e-13)
    np.testing.assert_allclose(b.kinetic_energy, a.kinetic_energy, rtol=1e-12)


JOURNAL_126 = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: 126, dx: 2.e-5, dy: 2.e-5, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 10., V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-8, dt: 1e-10, max_it: 10000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, T0: 323.15, C1: 3.5e10, C2: 1.23}}
"""


def test_largest_shape_and_the_first_refused(hiplib):
    """6. 126 x 126 (16384 cells, 32 per thread), 3 steps, against the oracle at FIELD_RTOL; 127 x 126 is refused by Python and
    by the library, by name."""
    from gapflow_amd import Ensemble, Problem
    from oracle.problem import OracleProblem
    text = JOURNAL_126.format(nx=126)
    p = quiet(Problem.from_string, text)
    quiet(p._pre_run)
    ens = Ensemble([p])
    assert ens.tiers == ['workspace']
    quiet(ens.step, 3)
    ref = quiet(OracleProblem.from_string, text)
    quiet(ref._pre_run)
    for _ in range(3):
        quiet(ref.update)
    assert p.step == ref.step == 3
    err = comp_err(p.q, ref.q)
    print(f'\n[126 x 126, 3 steps] err against the oracle {err}')
    assert (err <= FIELD_RTOL).all(), err
    np.testing.assert_allclose(p.dt, ref.dt, rtol=1e-10)

    big = quiet(Problem.from_string, JOURNAL_126.format(nx=127))
    with pytest.raises(NotImplementedError, match=r"member 1: .*127 x 126.*LDS"):
        Ensemble([p, big])
    e = C.c_void_p()
    handles = (C.c_void_p * 2)(p._h.value, big._h.value)
    for rc in (hiplib.gpf_ensemble_create(handles, 2, C.byref(e)), hiplib.gpf_ensemble_create2(handles, 2, 1, C.byref(e))):
        msg = hiplib.gpf_last_error().decode()
        assert rc != 0 and 'member 1' in msg and 'LDS' in msg and '16384' in msg
    cells, per_cell = C.c_int64(0), C.c_int32(0)
    assert hiplib.gpf_ensemble_limits2(C.byref(cells), C.byref(per_cell)) == 0
    from gapflow_amd import _lib
    assert (cells.value, per_cell.value) == (_lib.MID_GRID_MAX_CELLS, _lib.MID_GRID_DOUBLES_PER_CELL) == (16384, 19)


def test_members_stop_on_their_own(hiplib):
    """7a. One run(): a loose tol converges early, a small max_it stops on it, an absurd dt is rolled back to the last valid
    state (as test_invalid_state_rolls_back provokes it: a numerical rollback), one member goes its 60 steps.  The neighbours of
    the invalid member are bit for bit what they are without it."""
    from gapflow_amd import Ensemble
    texts = [journal(40, ny=40, U=10., tol='1e-1', max_it=60), journal(50, ny=50, U=10., max_it=23),
             journal(40, ny=40, U=10., eps=0.5, max_it=60), journal(44, ny=36, U=10., eps=0.5, max_it=60)]

    def prepared(which):
        ps = {m: build(texts[m]) for m in which}
        if 2 in ps:
            quiet(ps[2].update)
            ps[2]._lib.gpf_set_dt(ps[2]._h, 1.0)        # absurd time step -> negative densities in the next one
            ps[2].dt = 1.0
        return ps

    ps = prepared(range(4))
    good = ps[2].q.copy()
    quiet(Ensemble(list(ps.values())).run)
    assert ps[0].converged and 1 <= ps[0].step < 23
    assert ps[1].step == 23 and not ps[1].converged and not ps[1]._stop
    assert ps[2]._stop and ps[2].step == 1
    np.testing.assert_array_equal(ps[2].q, good)
    assert ps[3].step == 60 and not ps[3]._stop
    without = prepared((0, 1, 3))
    quiet(Ensemble(list(without.values())).run)
    for m in (0, 1, 3):
        assert_same_member(ps[m], state_of(without[m]), f"member {m} with and without the invalid neighbour")


def test_a_member_goes_on_alone(hiplib):
    """7b. journal2d_periodic50_u10 through 10 ensemble steps, then 10 update() alone (k_step2, which redoes the predictor from
    the previous state the ensemble kernel left): the step-20 golden within field_tol."""
    from gapflow_amd import Ensemble
    p, fx, meta = make_problem('journal2d_periodic50_u10')
    other = make_problem('slider2d_dn')[0]
    quiet(Ensemble([other, p]).step, 10)
    assert p.step == 10
    for _ in range(10):
        quiet(p.update)
    tol = field_tol(fx, 20)
    err = comp_err(p.q, fx['q_20'])
    print(f'\n[journal2d_periodic50_u10] 10 ensemble steps + 10 alone: err {err} tol {tol}')
    assert (tol <= 1e-8).all() and (err <= tol).all(), f'err {err} tol {tol}'
    check_history(fx['history'][19], p, history_tol(fx))
