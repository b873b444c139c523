"""The case table of tests/test_gpu_validity.py against what it claims, on the oracle alone: every shape takes the kernel its
case names; the fixed time step moves no planted quantity by more than a per cent of its distance to the threshold it is meant
to cross; a planted maximum is at least twice the runner-up after the step; the planted densities have the sound speeds and
pressures the table states; after one step of a planted invalid state exactly the planted cell, its rule images and (for a NaN)
the stencil neighbours of the two stages are NaN or negative; and every planted case is discriminating -- without the planted
cell the oracle decides otherwise.  (The oracle steps a handful of positions per case: corners, edge middles, the centre.)"""
import numpy as np
import pytest

import validity_cases as V

ALL_CASES = {c.id: c for c in V.MAX_CASES + V.SOUND_CASES + V.INVALID_CASES}


def probes(case):
    nx, ny = case.nx, case.ny
    return sorted({(1, 1), (nx, ny), (1, (ny + 1) // 2), ((nx + 1) // 2, ny), ((nx + 1) // 2, (ny + 1) // 2)})


def v_of(q):
    with np.errstate(all='ignore'):
        return (q[1]**2 + q[2]**2) / q[0]


def test_table_is_what_it_says():
    from gapflow_amd import _lib
    assert all(_lib.EOS_IDS[law] == V.M.EOS_ID[law] for law in V.PROPS)
    assert len(ALL_CASES) == len({c.id for c in ALL_CASES.values()})
    for cases, laws in ((V.MAX_CASES, {'DH', 'BWR'}), (V.SOUND_CASES, {'vdW', 'BWR'}), (V.INVALID_CASES, {'DH'})):
        assert {c.law for c in cases} == laws and sorted(V.HEAVY[l] for l in laws) in ([False, True], [False])
        step2 = [c for c in cases if c.path == 'k_step2']
        assert {(c.law, c.variant, c.nx, c.ny, c.chunks) for c in step2} == {(l, v) + s for l in laws for v in V.VARIANTS for s in V.STEP2_SHAPES}
        for law in laws:
            assert {c.bc for c in step2 if c.law == law} == {'pp', 'dd'}
            assert {(c.nx, c.ny) for c in cases if c.path == 'k_small_steps' and c.law == law} == set(V.SMALL_SHAPES)
            assert {c.path for c in cases if c.law == law} == set(V.PATHS)
    # which kernel takes which shape: one workgroup's LDS holds 1200 cells, ghost cells included (small_grid_fits_lds)
    for c in ALL_CASES.values():
        assert ((c.nx + 2) * (c.ny + 2) <= V.ONE_WORKGROUP_CELLS) == (c.path == 'k_small_steps'), c.id
        assert c.chunks == (2 if (c.nx, c.ny) == (230, 20) else 0) and (not c.chunks or c.nx // c.chunks >= 100)
    assert (V.ENSEMBLE_SHAPES['lds'][0] + 2) * (V.ENSEMBLE_SHAPES['lds'][1] + 2) <= V.ONE_WORKGROUP_CELLS
    # parts 1 - 3 hold no exact zero of density
    for kinds, cases in ((V.KINDS_MAX, V.MAX_CASES), (V.KINDS_SOUND, V.SOUND_CASES), (V.KINDS_INVALID, V.INVALID_CASES)):
        for c in (cases[0], [x for x in cases if x.bc == 'dd'][0]):
            for kind in kinds:
                if kind in V.NEEDS_EDGE and c.bc != 'dd':
                    continue
                assert (V.plant(c, kind, (1, 1))[0] != 0.).all()
    # the seams the positions of part 3 are there for
    c14, c230 = (next(c for c in V.INVALID_CASES if (c.nx, c.ny) == s) for s in ((14, 130), (230, 20)))
    assert {(7, 126), (7, 127), (7, 130)} <= set(V.invalid_positions(c14)) and {(115, 10), (116, 10)} <= set(V.invalid_positions(c230))
    # every row of every k_step2 shape is planted (14 x 130: in both strips), so whatever the plan every wave of every block is met
    for c in (c for c in V.INVALID_CASES if c.path != 'k_small_steps'):
        cols = {iy for _, iy in V.row_sweep(c)}
        assert all({ix for ix, iy in V.row_sweep(c) if iy == col} == set(range(1, c.nx + 1)) for col in cols)
        for nchunks in range(1, c.nx // 4 + 1):         # and the far pair lies in the first and the last wave of any plan
            for D in (1, -1):
                (b0, w0), (b1, w1) = (V.wave_of(c, nchunks, pos, D) for pos in V.far_pair(c))
                nwaves = nchunks * -(-c.ny // V.STRIP_COLUMNS)
                assert {w0, w1} == {0, nwaves - 1} and {b0, b1} == {0, (nwaves - 1) // 4}
                assert {V.wave_of(c, nchunks, pos, D)[1] for pos in V.row_sweep(c)} == set(range(nwaves))


def test_slab_jobs_decide():
    """The slab cases: a cell in each rank in turn, on a row its neighbour reads and away from it; every one stops the oracle."""
    from gapflow_amd.slab import partition
    import edge_rule_cases as E
    case = V.SLAB_CASE
    assert (case.nx, case.ny) == E.SLAB_SHAPE and case.law == 'DH'
    bounds = [tuple(b) for b in partition(case.nx, V.SLAB_RANKS)]
    jobs = V.slab_jobs(case, bounds)
    seams = {hi for lo, hi in bounds[:-1]} | {lo for lo, hi in bounds[1:]}
    for r, (lo, hi) in enumerate(bounds):
        mine = [cells[0] for label, q, cells in jobs if label.startswith(f'rank {r}:')]
        assert all(lo <= ix <= hi for ix, iy in mine)
        assert any(ix in seams for ix, iy in mine) and any(ix not in seams and lo < ix < hi for ix, iy in mine)
    assert not V.oracle_outcome(case, V.base_state(case))['stopped']
    codes = set()
    for k, (label, q, cells) in enumerate(jobs):
        out = V.oracle_outcome(case, q, k % 2)
        assert out['stopped'] and out['step'] == k % 2, label
        assert out['invalid'] == (2 if 'nan' not in label and 'zero' not in label else 1), label
        codes.add(out['invalid'])
    assert codes == {1, 2}


def test_fill_ghosts_is_the_oracles_ghost_fill():
    from oracle.problem import OracleProblem
    rng = np.random.default_rng(3)
    for case in (V.MAX_CASES[0], next(c for c in V.MAX_CASES if c.bc == 'dd'), next(c for c in V.MAX_CASES if c.path == 'k_small_steps' and c.bc == 'dd')):
        p = V.make(OracleProblem, case)
        q = rng.uniform(1., 7., p.q.shape)
        p.q[...] = q
        p.communicate_ghost_buffers()
        np.testing.assert_array_equal(V.fill_ghosts(q.copy(), case), p.q, err_msg=case.id)
        # the base state is its own ghost fill, and a planted cell shows in exactly its images
        base = V.base_state(case)
        np.testing.assert_array_equal(V.fill_ghosts(np.array(base), case), base)
        for pos in probes(case):
            diff = np.argwhere((V.plant(case, 'negative', pos) != base).any(0))
            assert sorted(map(tuple, diff)) == V.images_of(case, pos), (case.id, pos)


def test_planted_densities_have_the_stated_sound_speeds():
    for law in V.SPINODAL:
        rho0, rho = V.RHO0[law], V.SPINODAL[law]
        assert np.isfinite(V.sound_speed(law, rho0)) and V.sound_speed(law, rho0) > 0. and np.isfinite(V.pressure(law, rho0))
        assert np.isnan(V.sound_speed(law, rho)) and np.isfinite(V.pressure(law, rho))
        # the image variant: a stable interior density whose Dirichlet image is the spinodal density, for every target
        for f in V.M.DD_FRACTIONS:
            inner = 2. * f * rho0 - rho
            assert inner > 0. and np.isfinite(V.sound_speed(law, inner)) and np.isfinite(V.pressure(law, inner))
            assert (2. * f * rho0 - inner) == pytest.approx(rho, rel=1e-12)
    # Dowson-Higginson: c^2 is a square, and a negative density stays finite in the closures
    assert np.isfinite(V.sound_speed('DH', -V.RHO0['DH'])) and np.isfinite(V.pressure('DH', [-V.RHO0['DH'], 0., 2.2 * V.RHO0['DH']])).all()


@pytest.mark.parametrize('cid', [c.id for c in V.MAX_CASES])
def test_planted_maximum_decides(cid):
    case = ALL_CASES[cid]
    base = V.base_state(case)
    plain = V.oracle_outcome(case, base)
    assert not plain['stopped'] and np.isfinite(plain['q']).all()
    kinds = ('spike',) + (('below', 'above') if case.bc == 'dd' else ())
    for kind in kinds:
        for pos in probes(case) if kind == 'spike' else [p for p in probes(case) if p in V.edge_cells(case)]:
            q = V.plant(case, kind, pos)
            out = V.oracle_outcome(case, q)
            what = f'{cid}: {kind} at {pos}'
            assert not out['stopped'] and out['step'] == 1 and (out['q'][0] > 0.).all(), what
            images = V.images_of(case, pos)
            v0, v1 = v_of(q), v_of(out['q'])
            others = np.ones(v0.shape, bool)
            for c in images:
                others[c] = False
            top0, top1 = max(v0[c] for c in images), max(v1[c] for c in images)
            assert top1 >= 2. * v1[others].max() and top0 >= 2. * v0[others].max(), what
            assert tuple(np.unravel_index(np.argmax(v1), v1.shape)) in images, what
            # the time step: v of the planted cell moves by less than a per cent of its distance to twice the runner-up
            assert abs(v1[pos] - v0[pos]) <= 0.01 * (v0[pos] - 2. * v0[others].max()), what
            if kind in ('below', 'above'):      # the density moves by less than a per cent of its distance to each adjacent target
                for t in V.adjacent_targets(case, pos):
                    assert abs(out['q'][0][pos] - q[0][pos]) <= 0.01 * abs(q[0][pos] - t), what
                holder = tuple(np.unravel_index(np.argmax(v1), v1.shape))
                assert (holder != pos) if kind == 'above' else (holder == pos or len(images) > 2), what
            # discriminating: without the planted cell all three records differ by far more than the tolerances
            assert abs(out['v_max'] / plain['v_max'] - 1.) > 0.4 and abs(out['ekin'] / plain['ekin'] - 1.) > 1e-6, what


@pytest.mark.parametrize('cid', [c.id for c in V.SOUND_CASES])
def test_planted_imaginary_sound_speed_decides(cid):
    case = ALL_CASES[cid]
    plain = V.oracle_outcome(case, V.base_state(case))
    assert not plain['stopped'] and np.isfinite(plain['v_sound'])          # the control
    edge = V.spinodal_edge(case.law, V.SPINODAL[case.law], V.RHO0[case.law])
    assert abs(V.spinodal_edge(case.law, V.SPINODAL[case.law], V.SPINODAL_FAR[case.law]) - V.SPINODAL[case.law]) > abs(edge - V.SPINODAL[case.law])
    for kind in ('spinodal',) + (('image',) if case.bc == 'dd' else ()):
        for pos in probes(case) if kind == 'spinodal' else [p for p in probes(case) if p in V.edge_cells(case)]:
            q = V.plant(case, kind, pos)
            out = V.oracle_outcome(case, q)
            what = f'{cid}: {kind} at {pos}'
            assert not out['stopped'] and out['step'] == 1 and np.isnan(out['v_sound']) and np.isfinite(out['ekin']), what
            assert np.isfinite(out['q']).all() and (out['q'][0] > 0.).all(), what
            c0, c1 = V.sound_speed(case.law, q[0]), V.sound_speed(case.law, out['q'][0])
            images = V.images_of(case, pos)
            holders = sorted(map(tuple, np.argwhere(np.isnan(c1))))
            assert holders == sorted(map(tuple, np.argwhere(np.isnan(c0)))) and set(holders) <= set(images), what
            assert (pos in holders) == (kind == 'spinodal'), what
            for c in holders:       # the time step: a per cent of the distance to the nearer edge of the spinodal
                assert abs(out['q'][0][c] - q[0][c]) <= 0.01 * abs(q[0][c] - edge), what
            # the next, unplanted step has a real sound speed again
            assert np.isfinite(V.oracle_outcome(case, V.base_state(case), 1)['v_sound'])


@pytest.mark.parametrize('cid', [c.id for c in V.INVALID_CASES])
def test_planted_invalid_cell_decides(cid):
    case = ALL_CASES[cid]
    base = V.base_state(case)
    assert not V.oracle_outcome(case, base)['stopped']          # without the planted cell the step commits
    rho0 = V.RHO0[case.law]
    for kind in V.KINDS_INVALID + ('zero',):
        cells = probes(case) if kind not in V.NEEDS_EDGE else [p for p in probes(case) if p in V.edge_cells(case)]
        if kind in V.NEEDS_EDGE and case.bc != 'dd':
            continue
        for pos in cells:
            q = V.plant(case, kind, pos)
            out = V.oracle_outcome(case, q)
            what = f'{cid}: {kind} at {pos}'
            assert out['stopped'] and out['step'] == 0, what
            np.testing.assert_array_equal(out['q'], q)
            j = out['judged']
            bad = {tuple(c) for c in np.argwhere(np.isnan(j).any(0) | (j[0] < 0.))}
            images = set(V.images_of(case, pos))
            if kind in ('negative', 'ghost-negative'):
                assert out['invalid'] == 2 and not np.isnan(j).any(), what
                assert bad == ({c for c in images if q[0][c] < 0.}), what
                for c in bad:       # the time step: a per cent of the distance to zero
                    assert abs(j[0][c] - q[0][c]) <= 0.01 * abs(q[0][c]), what
            else:                   # a NaN (the zero density makes one in the closures): the cell, its images, and what two stages reach
                assert out['invalid'] == 1 and images <= bad, what
                reach = {(a + da, b + db) for a, b in images for da in range(-2, 3) for db in range(-2, 3)}
                wrap = {(a % (case.nx + 2), b % (case.ny + 2)) for a, b in reach} | {((a - 1) % case.nx + 1, (b - 1) % case.ny + 1) for a, b in reach}
                near = set()
                for a, b in wrap:
                    near |= set(V.images_of(case, (min(max(a, 1), case.nx), min(max(b, 1), case.ny)))) | {(a, b)}
                assert bad <= near, f'{what}: NaN at {sorted(bad - near)}'
            good = np.array([[c not in bad for c in ((a, b) for b in range(case.ny + 2))] for a in range(case.nx + 2)])
            assert (j[0][good] > 0.5 * rho0).all(), what
    # a NaN and a negative density far apart: the NaN decides the code
    a, b = V.far_pair(case)
    if a != b:
        out = V.oracle_outcome(case, V.plant(case, 'negative', b, V.plant(case, 'nan-jy', a)))
        assert out['stopped'] and out['invalid'] == 1
        assert a[0] != b[0] or a[1] != b[1]
