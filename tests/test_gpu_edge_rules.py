"""Every ghost-cell rule triple on every step path (tests/edge_rule_cases.py: per axis one of the eight D/N triples of (rho, jx,
jy) or all-periodic, 81 pairs, four unequal targets), six steps against the oracle.  The paths and how each is forced:

  k_step2 (ghost_rule: the in-march x and y ghosts, the closing ghost pass, the corners)   14 x 130 and 37 x 40, all 81 pairs
  the split form (k_ghost_stage1 / k_ghost_fill: ghost_fill_block)   GPF_STEP_UNFUSED_EDGES=1 before the handle is created
  the reference-ordered pipeline (k_bc_x / k_bc_y)                    gpf_step_unfused
  the stage-wise pipeline of Problem.update() (k_bc_x / k_bc_y)       a shear-thinning law, which the fused kernel refuses
  k_small_steps (the `ghosts` lambda)       9 x 20 (all 81), 30 x 1 and 1 x 30 (the axis' nine triples, the other axis periodic)
  k_mid_ensemble (its twin)                 Ensemble(..., tier='workspace') at 37 x 40
  the slab edge items (step_kernel.hip)     3 ranks as threads (ThreadWorld: the all-gather transport, the only one it has)
  the ghost fill behind gpf_resample        init_from, against reference_ghosts of the new interior
  checkpoints                               the rules travel with the file

Tolerances are test_gpu_ragged.run_case's: fields within 1e-9 of each component's scale over the whole ghosted array, corners
included; dt and the kinetic energy to rtol 1e-9, the mass to 1e-12.  tests/test_edge_rules_host.py shows on the oracle alone that
every case here is conditioned ten times better than that and that a swapped target or a rule read from another component moves
the result by more than 1e-6."""
import ctypes as C

import numpy as np
import pytest

import edge_rule_cases as E

pytestmark = pytest.mark.gpu

FIELD_TOL, SCALAR_RTOL, MASS_RTOL = 1e-9, 1e-9, 1e-12
IDS = [E.pair_id(p) for p in E.PAIRS]
IDS16 = [E.pair_id(p) for p in E.SIXTEEN]


@pytest.fixture(autouse=True)
def fused_unless_asked(monkeypatch):
    monkeypatch.delenv('GPF_STEP_UNFUSED_EDGES', raising=False)


def ran_k_step2(prob):
    """gpf_step_variant answers only on a handle that has launched the fused step kernel."""
    return prob._lib.gpf_step_variant(prob._h, (C.c_int * 5)()) == 0


def check(label, pair, shape, q, dt, ekin, mass, ref, rows=slice(None)):
    """q (rows `rows` of the domain) and the scalars against the oracle's run, at run_case's tolerances."""
    scale = np.array([np.abs(c).max() or 1. for c in ref['q']])
    errs = np.array([np.abs(q[c] - ref['q'][c, rows]).max() / scale[c] for c in range(3)])
    print(f'\n[{label} {shape[0]} x {shape[1]} {E.pair_id(pair)} MC_order {E.mc_order_of(pair)}] max error of (rho, jx, jy) after {E.STEPS} steps: '
          + ', '.join(f'{e:.1e}' for e in errs) + f' of scale (tolerance {FIELD_TOL:g}); relative error of dt {abs(dt / ref["dt"] - 1):.1e}, '
          f'ekin {abs(ekin / ref["ekin"] - 1):.1e}, mass {abs(mass / ref["mass"] - 1):.1e}')
    for c in range(3):
        assert errs[c] <= FIELD_TOL, f'{label}, {E.pair_id(pair)}: component {c}: {errs[c]:.3e}'      # ghost cells and corners included
    np.testing.assert_allclose(dt, ref['dt'], rtol=SCALAR_RTOL, err_msg=label)
    np.testing.assert_allclose(ekin, ref['ekin'], rtol=SCALAR_RTOL, err_msg=label)
    np.testing.assert_allclose(mass, ref['mass'], rtol=MASS_RTOL, err_msg=label)
    return errs


def stepped(pair, shape, **text_args):
    """A Problem of the case after six update()s, and the oracle's run; the initial fields are the same bits."""
    from gapflow_amd import Problem
    ref = E.oracle_run(pair, shape, text_args.get('thinning', False))
    gpu = E.make(Problem, pair, shape, **text_args)
    np.testing.assert_array_equal(gpu.q, ref['q0'])
    for _ in range(E.STEPS):
        gpu.update()
    assert gpu.step == ref['steps'] == E.STEPS
    return gpu, ref


_FUSED = {}


def fused_run(pair, shape):
    """k_step2's own result of a case (q, dt), computed once and left unchanged."""
    key = (tuple(pair), tuple(shape))
    if key not in _FUSED:
        gpu, _ = stepped(pair, shape)
        assert ran_k_step2(gpu)
        q = gpu.q.copy()
        q.setflags(write=False)
        _FUSED[key] = (q, gpu.dt)
    return _FUSED[key]


# ---- k_step2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', E.STEP2_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('pair', E.PAIRS, ids=IDS)
def test_fused_step_kernel(hiplib, pair, shape):
    gpu, ref = stepped(pair, shape)
    assert ran_k_step2(gpu), 'the case was meant for k_step2'
    check('k_step2', pair, shape, gpu.q, gpu.dt, gpu.kinetic_energy, gpu.mass, ref)


# ---- the split form and the two pipelines -------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', E.SIXTEEN, ids=IDS16)
def test_split_edge_form(hiplib, monkeypatch, pair):
    """k_ghost_stage1 before and k_ghost_fill behind a k_step2 that does no edge work: against the oracle, and bit for bit the fused
    form's field and dt (Dowson-Higginson: what test_split_edge_form_records_the_same_series and
    test_fused_slab_step_is_bitwise_the_split_step hold the two forms to; the kinetic energy is summed in another order)."""
    shape = E.MID_SHAPE
    q_fused, dt_fused = fused_run(pair, shape)
    monkeypatch.setenv('GPF_STEP_UNFUSED_EDGES', '1')           # read by gpf_create
    gpu, ref = stepped(pair, shape)
    assert ran_k_step2(gpu)
    q = gpu.q
    check('split form', pair, shape, q, gpu.dt, gpu.kinetic_energy, gpu.mass, ref)
    assert np.array_equal(q, q_fused), f'{np.abs(q - q_fused).max():.3e} away from the fused form'
    assert gpu.dt == dt_fused


@pytest.mark.parametrize('pair', E.SIXTEEN, ids=IDS16)
def test_reference_ordered_pipeline(hiplib, pair):
    """gpf_step_unfused: one kernel per reference function, k_bc_x / k_bc_y after each stage and after the average."""
    from gapflow_amd import Problem, _lib
    shape = E.MID_SHAPE
    ref = E.oracle_run(pair, shape)
    gpu = E.make(Problem, pair, shape)
    for _ in range(E.STEPS):
        gpu._sync_to_device()
        _lib.check(hiplib.gpf_step_unfused(gpu._h))
        gpu._mark_device_advanced()
    sc = gpu._scalars()
    assert sc.step == E.STEPS and not sc.invalid and not ran_k_step2(gpu)
    check('reference-ordered pipeline', pair, shape, gpu.q, sc.dt, sc.ekin, sc.mass, ref)


@pytest.mark.parametrize('pair', E.SIXTEEN, ids=IDS16)
def test_stage_wise_pipeline_with_shear_thinning(hiplib, pair):
    """Problem.update() of a problem the fused kernel cannot take (the viscosity needs grad p)."""
    shape = E.MID_SHAPE
    gpu, ref = stepped(pair, shape, thinning=True)
    assert gpu._cfg.thinning and not ran_k_step2(gpu)
    assert gpu._lib.gpf_step(gpu._h, 1, 0, None, 0, C.byref(C.c_int64())) == -5        # the fused entry point refuses it
    check('stage-wise pipeline, Carreau', pair, shape, gpu.q, gpu.dt, gpu.kinetic_energy, gpu.mass, ref)


# ---- one workgroup ------------------------------------------------------------------------------------------------------------
SMALL = ([(p, E.SMALL_SHAPE) for p in E.PAIRS] + [(p, E.ROW_SHAPE) for p in E.row_pairs()] + [(p, E.COLUMN_SHAPE) for p in E.column_pairs()])


@pytest.mark.parametrize('pair,shape', SMALL, ids=[f'{E.pair_id(p)}-{s[0]}x{s[1]}' for p, s in SMALL])
def test_one_workgroup_kernel(hiplib, pair, shape):
    gpu, ref = stepped(pair, shape)
    assert not ran_k_step2(gpu), 'the case was meant for k_small_steps'
    check('k_small_steps', pair, shape, gpu.q, gpu.dt, gpu.kinetic_energy, gpu.mass, ref)


def test_workspace_tier_ensemble(hiplib):
    """The sixteen pairs as the members of one ensemble, each against its own oracle run."""
    from gapflow_amd import Ensemble, Problem
    shape = E.MID_SHAPE
    ps = [E.make(Problem, pair, shape) for pair in E.SIXTEEN]
    ens = Ensemble(ps, tier='workspace')
    assert ens.tiers == ['workspace'] * len(ps)
    ens.step(E.STEPS)
    for pair, p in zip(E.SIXTEEN, ps):
        assert p.step == E.STEPS and not ran_k_step2(p)
        check('k_mid_ensemble', pair, shape, p.q, p.dt, p.kinetic_energy, p.mass, E.oracle_run(pair, shape))


# ---- slabs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', E.SLAB_PAIRS, ids=[E.pair_id(p) for p in E.SLAB_PAIRS])
def test_three_slabs(hiplib, pair):
    """Three x-slabs (13 + 12 + 12 rows; the physical x edges on ranks 0 and 2, the y edges on all): every rank's rows with their
    outer rows against the oracle; its own rows bit for bit the undivided Problem's and the same dt on every rank (the relation
    test_n_slabs_are_bitwise_the_one_slab_run asserts)."""
    import torch
    from gapflow_amd import _lib
    from gapflow_amd.slab import SlabProblem, ThreadWorld
    shape = E.SLAB_SHAPE
    ref = E.oracle_run(pair, shape)
    q_serial, dt_serial = fused_run(pair, shape)
    text = E.case_text(pair, shape)

    def rank_body(group):
        slab = SlabProblem.from_string(text, device=0, dist=group)
        slab.pre_run()                                      # dt of the uniform state, as E.make
        L = slab.layout
        slab._upload(_lib.FIELD_Q, ref['q0'][:, L.lo - 1:L.hi + 2])
        _lib.check(slab.lib.gpf_set_ekin_old(slab._h, float(slab.global_scalars()['ekin'])))
        slab.advance(E.STEPS)
        st = slab.state()
        return L, slab.local_q(), (int(st.step), int(st.invalid), st.dt, st.ekin, slab.global_scalars()['mass'])

    runs = ThreadWorld(3, torch).run(rank_body)
    assert sum(L.nx for L, _, _ in runs) == shape[0]
    for L, q, (step, invalid, dt, ekin, mass) in runs:
        assert step == E.STEPS and invalid == 0
        check(f'slab {L.rank} of 3', pair, shape, q, dt, ekin, mass, ref, rows=slice(L.lo - 1, L.hi + 2))
        own = q_serial[:, L.lo:L.hi + 1]
        assert np.array_equal(q[:, 1:-1], own), f'rank {L.rank}: {np.abs(q[:, 1:-1] - own).max():.3e} away from the undivided run'
        assert dt == dt_serial, f'rank {L.rank}: dt {dt!r} vs {dt_serial!r}'


# ---- init_from, checkpoints, refusals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', [('NDD', 'DNN'), ('NNN', 'DND')], ids=E.pair_id)
def test_init_from_fills_ghosts_by_the_new_rules(hiplib, pair):
    """A coarse 15 x 13 state onto 37 x 40: the ghost cells gpf_resample leaves are reference_ghosts of the new interior, to the
    1e-13 of each component's largest magnitude test_gpu_resample.py holds ghost cells to."""
    from gapflow_amd import Problem
    fine, coarse = (37, 40), (15, 13)
    lengths = (fine[0] * 2.e-5, fine[1] * 2.5e-5)
    src = E.make(Problem, pair, coarse, lengths=lengths)
    for _ in range(3):
        src.update()
    dst = E.make(Problem, pair, fine, lengths=lengths)
    before = dst.q.copy()
    dst.init_from(src)
    got = np.array(dst.q)
    assert np.isfinite(got).all() and not np.array_equal(got[:, 1:-1, 1:-1], before[:, 1:-1, 1:-1])
    want = E.reference_ghosts(got, E.rules_of(pair), E.targets_of(pair))
    for c, name in enumerate(('rho', 'jx', 'jy')):
        scale = np.abs(want[c]).max()
        err = np.abs(got[c] - want[c]).max()
        print(f'\n[init_from {E.pair_id(pair)}] {name}: ghost cells {err / scale:.1e} of max|{name}| away from the rules (tolerance 1e-13)')
        assert err <= 1e-13 * scale, f'{name}: {err:.3e} > 1e-13 x {scale:.3e}'
    # each Dirichlet ghost differs from its neighbour, so the check above saw the targets
    assert (got[1, 0, 1:-1] != got[1, 1, 1:-1]).all() if pair[0][1] == 'D' else (got[1, 0, 1:-1] == got[1, 1, 1:-1]).all()


def test_checkpoint_carries_the_rules(hiplib, tmp_path):
    """DDN x NND at 37 x 40: saved after 3 steps and continued for 3 is bit for bit the uninterrupted run; the restored problem
    holds the same rules and targets."""
    from gapflow_amd import Problem
    pair, shape = ('DDN', 'NND'), (37, 40)
    q_whole, dt_whole = fused_run(pair, shape)
    a = E.make(Problem, pair, shape)
    for _ in range(3):
        a.update()
    path = str(tmp_path / 'edge.gpf')
    a.save_checkpoint(path)
    b = Problem.from_checkpoint(path)
    assert b.step == 3 and b._edge_rules() == a._edge_rules()
    assert [list(r) for r in b._cfg.bc_rule] == [list(r) for r in a._cfg.bc_rule] == b._edge_rules()[0]
    assert list(b._cfg.bc_value) == list(a._cfg.bc_value) == b._edge_rules()[1]
    for _ in range(3):
        b.update()
    assert b.step == E.STEPS and b.dt == dt_whole
    assert np.array_equal(b.q, q_whole), f'{np.abs(b.q - q_whole).max():.3e} away from the uninterrupted run'
    check('restored, k_step2', pair, shape, b.q, b.dt, b.kinetic_energy, b.mass, E.oracle_run(pair, shape))


def test_unequal_opposite_edges_and_partly_periodic_edges_are_refused(hiplib):
    from gapflow_amd import Problem
    text = E.case_text(('DNN', 'NDN'), (9, 20))
    Problem.from_string(text)
    with pytest.raises(NotImplementedError, match='opposite edges must declare the same D/N types'):
        Problem.from_string(text.replace("xW: ['D', 'N', 'N']", "xW: ['N', 'D', 'N']"))
    with pytest.raises(NotImplementedError, match='opposite edges must declare the same D/N types'):
        Problem.from_string(text.replace("yN: ['N', 'D', 'N']", "yN: ['N', 'N', 'N']"))
    partly = text.replace("xE: ['D', 'N', 'N']", "xE: ['D', 'P', 'N']").replace("xW: ['D', 'N', 'N']", "xW: ['D', 'P', 'N']")
    assert partly != text
    with pytest.raises(NotImplementedError, match='periodic for all components or for none'):
        Problem.from_string(partly)
