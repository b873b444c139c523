"""The case table of tests/test_gpu_edge_rules.py against what it claims, on the oracle alone: the oracle's ghost fill is the
cell-by-cell restatement of the reference's for every pair of rule triples; every case the GPU test runs finishes its six steps
on a valid state and is conditioned well enough for the 1e-9 comparison to be a real check; and that comparison could see a
target taken from the wrong side or a rule taken from the wrong component."""
import numpy as np
import pytest

import edge_rule_cases as E

SENS_BOUND = 1e-10      # a condition on the inputs: the 1e-9 field tolerance keeps a factor of 10 over the oracle's own conditioning
IDS = [E.pair_id(p) for p in E.PAIRS]


def gpu_cases():
    """Every (pair, shape, thinning) tests/test_gpu_edge_rules.py steps against the oracle."""
    cases = [(p, s, False) for p in E.PAIRS for s in E.STEP2_SHAPES + [E.SMALL_SHAPE]]
    cases += [(p, E.ROW_SHAPE, False) for p in E.row_pairs()] + [(p, E.COLUMN_SHAPE, False) for p in E.column_pairs()]
    cases += [(p, E.MID_SHAPE, True) for p in E.SIXTEEN]
    return cases


def test_table_is_what_it_says():
    assert len(E.TRIPLES) == 9 and len(set(E.TRIPLES)) == 9 and len(E.PAIRS) == 81
    assert set(E.DN_TRIPLES) == {a + b + c for a in 'DN' for b in 'DN' for c in 'DN'}
    assert len(E.SIXTEEN) == 16 == len(set(E.SIXTEEN)) and set(E.SIXTEEN) <= set(E.PAIRS)
    assert {mc for mc in map(E.mc_order_of, E.PAIRS)} == {1, -1, 0} and {E.mc_order_of(p) for p in E.SIXTEEN} == {1, -1, 0}
    # the targets of a problem are all unequal
    for p in E.PAIRS:
        t = list(E.targets_of(p).values())
        assert len(set(t)) == len(t) == 2 * sum('D' in triple for triple in p)
    # the sixteen (the split form, both pipelines, the ensemble) are shapes k_step2 and the host test cover
    assert E.MID_SHAPE in E.STEP2_SHAPES and E.SLAB_SHAPE in E.STEP2_SHAPES
    # slabs: a non-periodic x triple with a D on a flux, and a y triple different from it
    assert len(E.SLAB_PAIRS) == 4 and set(E.SLAB_PAIRS) <= set(E.SIXTEEN)
    assert all(x != 'PPP' and 'D' in x[1:] and y != x for x, y in E.SLAB_PAIRS)
    # which kernel takes which shape: one workgroup's LDS holds 1200 cells, ghost cells included (small_grid_fits_lds)
    assert all((nx + 2) * (ny + 2) > 1200 for nx, ny in E.STEP2_SHAPES)
    assert all((nx + 2) * (ny + 2) <= 1200 for nx, ny in (E.SMALL_SHAPE, E.ROW_SHAPE, E.COLUMN_SHAPE))


@pytest.mark.parametrize('shape', [(5, 4), (1, 1)], ids=['5x4', '1x1'])
def test_oracle_ghost_fill_is_the_restatement(shape):
    """OracleProblem.communicate_ghost_buffers against reference_ghosts (plain loops, no code shared) on a random ghosted
    array, for all 81 pairs: equal exactly."""
    from oracle.problem import OracleProblem
    rng = np.random.default_rng(5)
    for pair in E.PAIRS:
        p = OracleProblem.from_string(E.case_text(pair, shape))
        q = rng.uniform(-3., 7., p.q.shape)
        p.q[...] = q
        p.communicate_ghost_buffers()
        np.testing.assert_array_equal(p.q[:, 1:-1, 1:-1], q[:, 1:-1, 1:-1])
        np.testing.assert_array_equal(p.q, E.reference_ghosts(q, E.rules_of(pair), E.targets_of(pair)), err_msg=E.pair_id(pair))


def test_restatement_sees_rule_value_and_corner_order():
    """The restatement itself, on the array 1..: a Dirichlet ghost is 2 target - adjacent with the side-swapped target, a Neumann
    ghost the adjacent cell, a corner rule_y(rule_x(.))."""
    q = np.arange(3 * 4 * 5, dtype=float).reshape(3, 4, 5)
    pair = ('DNN', 'NDN')
    t = E.targets_of(pair)
    g = E.reference_ghosts(q, E.rules_of(pair), t)
    assert g[0, 0, 2] == 2. * t['xW'] - q[0, 1, 2] and g[0, 3, 2] == 2. * t['xE'] - q[0, 2, 2]     # low x: xW's value
    assert g[1, 0, 2] == q[1, 1, 2] and g[2, 3, 2] == q[2, 2, 2]
    assert g[1, 1, 0] == 2. * t['yN'] - q[1, 1, 1] and g[1, 1, 4] == 2. * t['yS'] - q[1, 1, 3]     # low y: yN's value
    assert g[0, 1, 0] == q[0, 1, 1]
    assert g[0, 0, 0] == 2. * t['xW'] - q[0, 1, 1] and g[1, 3, 4] == 2. * t['yS'] - q[1, 2, 3]
    both = E.reference_ghosts(q, E.rules_of(('DDD', 'DDD')), E.targets_of(('DDD', 'DDD')))
    tt = E.targets_of(('DDD', 'DDD'))
    assert both[2, 0, 0] == 2. * tt['yN'] - (2. * tt['xW'] - q[2, 1, 1])


@pytest.mark.parametrize('pair', E.PAIRS, ids=IDS)
def test_every_gpu_case_is_valid_and_well_conditioned(pair):
    """No rollback, finite fields, rho > 0, and one ulp of density noise moves no component by more than 1e-10 of its scale."""
    for p, shape, thinning in gpu_cases():
        if p != pair:
            continue
        ref = E.oracle_run(p, shape, thinning)
        what = f'{E.pair_id(p)} at {shape[0]} x {shape[1]}' + (' with shear thinning' if thinning else '')
        assert ref['steps'] == E.STEPS and not ref['stopped'], what
        assert np.isfinite(ref['q']).all() and (ref['q'][0] > 0.).all(), what
        assert (ref['sens'] <= SENS_BOUND).all(), f"{what}: one ulp of density moves (rho, jx, jy) by {ref['sens']} of scale"
        # the wave: both fluxes vary along every edge of the initial state, and all three components have moved
        q0 = ref['q0']
        for c in (1, 2):
            for line in (q0[c, 1, :], q0[c, -2, :], q0[c, :, 1], q0[c, :, -2]):
                assert line.size <= 3 or np.ptp(line) > 1e-3 * np.abs(line).max(), what
        assert (E.field_err(ref['q'], q0) > 1e-6).all(), what


def exchanged(triple):
    """The triple with a D moved to another component, its targets still fit for it: the two fluxes' rules exchanged where they
    differ, DNN -> NDN (a density-like target on a flux, as DDx has it); None for DDD, NNN, PPP -- and for NDD, whose only move
    would put a flux-like target on the density."""
    if triple[1] != triple[2]:
        return triple[0] + triple[2] + triple[1]
    return 'NDN' if triple == 'DNN' else None


@pytest.mark.parametrize('pair', [p for p in E.PAIRS if 'D' in p[0] + p[1]], ids=lambda p: E.pair_id(p))
def test_the_comparison_could_see_a_wrong_value_or_a_wrong_component(pair):
    """Swapping the two targets of an axis, or exchanging which component carries the D (targets kept), changes the oracle's
    six-step result by more than 1e-6 of scale: a thousand times the 1e-9 the GPU test compares at."""
    shape = E.SMALL_SHAPE
    ref = E.oracle_run(pair, shape)
    t = E.targets_of(pair)
    for axis, sides in ((0, ('xE', 'xW')), (1, ('yS', 'yN'))):
        if 'D' not in pair[axis]:
            continue
        swapped = dict(t)
        swapped[sides[0]], swapped[sides[1]] = t[sides[1]], t[sides[0]]
        p, _ = E.oracle_steps(pair, shape, targets=swapped)
        assert p.step == E.STEPS and not p._stop
        assert E.field_err(p.q, ref['q']).max() > 1e-6, f'{E.pair_id(pair)}: targets of {sides} swapped'
        other = exchanged(pair[axis])
        if other is not None:
            moved = (other, pair[1]) if axis == 0 else (pair[0], other)
            p, _ = E.oracle_steps(moved, shape, targets=t, mc=E.mc_order_of(pair))
            assert p.step == E.STEPS and not p._stop
            assert E.field_err(p.q, ref['q']).max() > 1e-6, f'{E.pair_id(pair)}: {pair[axis]} -> {other} on axis {axis}'
