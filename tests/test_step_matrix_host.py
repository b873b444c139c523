"""The case table of tests/test_gpu_step_matrix.py against what it claims, on the oracle alone: every case is out of the
one-workgroup kernel's reach, runs its six steps on a valid state, is conditioned well enough for every component to be a real
check, moves, and exercises the branch or the viscosity law it is there for."""
import numpy as np
import pytest

from helpers import comp_err, field_tol
import step_matrix_cases as M


@pytest.mark.parametrize('case', M.CASES, ids=M.IDS)
def test_case_can_detect_what_it_claims(case):
    assert (case.nx + 2) * (case.ny + 2) > 1200         # small_grid_fits_lds: more than one workgroup's LDS holds
    ref = M.oracle_run(case)
    q, q0 = ref['q'], ref['q0']
    assert np.isfinite(q).all() and (q[0] > 0.).all()
    assert ref['steps'] == M.STEPS and not ref['stopped']       # no rollback
    tol = field_tol({'sens_end': ref['sens']}, 'end')
    assert (tol <= 1e-8).all(), f'conditioned to {tol} only'    # the cap test_fused_step_matches_golden enforces
    moved = comp_err(q, q0)
    assert (moved[1:] > 1e-6).all(), f'the fluxes moved by {moved[1:]} of their scale'
    if case.law == 'Bayada':            # the liquid branch and the mixture branch
        rho_l = ref['prop']['rho_l']
        assert q[0].min() < rho_l < q[0].max()
    if case.piezo in ('Barus', 'Roelands'):
        mu = ref['viscosity']
        assert (mu > 0.).all() and mu.max() - mu.min() > 0.01 * mu.mean()
    if case.piezo:
        assert ref['prop']['piezo']['name'] == case.piezo
    if 'slip' in case.variant:
        ls = M.slip_field(case, M.input_of(case)['grid'])
        assert ls.min() > 0. and ls.max() > 2. * ls.min()


def test_table_covers_the_matrix():
    from gapflow_amd import _lib
    assert M.EOS_ID == _lib.EOS_IDS and M.PIEZO_ID == _lib.PIEZO_IDS
    assert len(set(M.IDS)) == len(M.CASES)
    assert len(M.MATRIX) == 56 and {(c.law, c.variant) for c in M.MATRIX} == {(l, v) for l in M.LAWS for v in M.VARIANTS}
    assert all(c.chunks == 0 and (c.nx, c.ny) in M.SHAPES for c in M.MATRIX + M.LINE_HY)
    # shapes and boundary conditions alternate down the table; each law and each variant meets both of each
    for key in ('law', 'variant'):
        for name in {getattr(c, key) for c in M.MATRIX}:
            rows = [c for c in M.MATRIX if getattr(c, key) == name]
            assert {(c.nx, c.ny) for c in rows} == set(M.SHAPES) and {c.bc for c in rows} == {'pp', 'dd'}, name
    assert {c.piezo for c in M.MATRIX} == {None, 'Barus', 'Roelands', 'Dukler', 'McAdams'}
    assert all((c.piezo is not None) == ('piezo' in c.variant) for c in M.CASES)
    assert {c.piezo for c in M.MATRIX if c.law == 'Bayada' and c.piezo} == {'Dukler', 'McAdams'}
    assert any(c.piezo in ('Dukler', 'McAdams') and c.law != 'Bayada' for c in M.MATRIX)
    # TOPO 1 with dh/dy != 0: a light and a heavy law, x-only planes
    assert sorted(M.LAWS[c.law].heavy for c in M.LINE_HY) == [False, True]
    for c in M.LINE_HY:
        planes = M.planes_of(c, M.input_of(c)['grid'])
        assert (planes == planes[:, :, :1]).all() and np.abs(planes[2]).min() > 0.
    # y-line: planes that vary along y only
    for c in (c for c in M.MATRIX if c.variant == 'y-line'):
        planes = M.planes_of(c, M.input_of(c)['grid'])
        assert (planes == planes[:, :1, :]).all() and not planes[1].any() and np.ptp(planes[0]) > 0.
    # long marches: every wave marches >= 100 rows
    assert {(c.law, c.variant) for c in M.LONG} == {(l, v) for l in ('PL', 'MT', 'BWR', 'Bayada', 'DH') for v in ('coef', 'table')}
    assert all(c.nx // c.chunks >= 100 and (c.nx, c.ny) == M.LONG_SHAPE for c in M.LONG)
    assert [l for l in M.LAWS if M.LAWS[l].heavy] == ['PL', 'MT', 'BWR', 'Bayada']         # Step2Weight::heavy
