"""The fold that closes a time step -- lane -> wave -> block -> the last block -> commit_step in k_step2, the LDS word and
block_reduce in k_small_steps / k_small_ensemble / k_mid_ensemble, the ScalarPartial records of the two pipelines and the split
form -- with the maximum or the invalid cell planted at chosen positions (tests/validity_cases.py; tests/test_validity_host.py shows
on the oracle alone that every planted state decides what it claims to decide).  How each path is forced: test_gpu_edge_rules.py's
docstring; every test asserts which kernel ran.

  1  planted maximum, every interior cell, both predictor directions: the step's committed record (the scalar log entry; gpf_scalars
     behind the two pipelines) against oracle/problem.py's kinetic_energy, v_max, v_sound evaluated in NumPy fp64 on the downloaded
     field, at helpers.HISTORY_RTOL's entries; the NumPy argmax of v lies in the planted cell or one of its ghost images
  2  planted imaginary sound speed, every interior cell: the step commits with v_sound NaN and invalid 0, the next unplanted step
     reports a real v_sound
  3  planted NaN / negative density at the seams of strips, chunks and waves, against OracleProblem.update() of the same bits: the
     run stops, the step count stays, invalid is 1 / 2, q is bit for bit the planted q, the pressure behind the refused step is the
     oracle's on every cell that holds no planted value
  4  rho = jx = jy = 0 in one cell: whatever the oracle decides

Three x-slabs as threads (the flags travel in rec[3] of a message) take parts 3 and 4 with the cell planted in each rank in turn.
A 230 x 20 sweep is taken in three interleaved parts, one test each."""
import ctypes as C

import numpy as np
import pytest

from helpers import HISTORY_RTOL
from step_matrix_cases import environment
import validity_cases as V

pytestmark = pytest.mark.gpu

EKIN_RTOL, VSOUND_RTOL, VMAX_RTOL = HISTORY_RTOL[3], HISTORY_RTOL[5], HISTORY_RTOL[6]
PRESSURE_TOL = 1e-9     # of scale: test_gpu_parity.py's


@pytest.fixture(autouse=True)
def fused_unless_asked(monkeypatch):
    monkeypatch.delenv('GPF_STEP_UNFUSED_EDGES', raising=False)


def step_variant(prob):
    """The (EOS, HAS_LS, PIEZO, D, TOPO) of the last k_step2 launch, None on a handle that has launched none."""
    out = (C.c_int * 5)()
    return tuple(out) if prob._lib.gpf_step_variant(prob._h, out) == 0 else None


def take_step(gpu, case):
    """One step by the case's path; returns (the committed step's record or None, which kernel ran)."""
    from gapflow_amd import _lib
    before = gpu.step
    if case.path in ('unfused', 'stagewise'):
        lib, h = gpu._lib, gpu._h
        gpu._sync_to_device()
        sc = _lib.GpfScalars()
        if case.path == 'unfused':
            _lib.check(lib.gpf_step_unfused(h))
        else:                                       # Problem.update()'s own sequence for a shear-thinning law
            assert gpu._cfg.thinning and lib.gpf_step(h, 1, 0, None, 0, C.byref(C.c_int64())) == -5
            _lib.check(lib.gpf_open_step(h))
            for i in range(2):
                _lib.check(lib.gpf_stage_closures(h))
                _lib.check(lib.gpf_stage_advance(h, i))
            _lib.check(lib.gpf_close_step(h, C.byref(sc)))
        gpu._mark_device_advanced()
        if case.path == 'unfused':
            sc = gpu._scalars()
        gpu.step = int(sc.step)
        assert step_variant(gpu) is None, f'{case.id}: meant for the {case.path} pipeline, ran k_step2'
        return (sc if sc.step == before + 1 else None), case.path
    entries = gpu._advance(1, honor_stop=False)
    ran = step_variant(gpu)
    if case.path == 'k_small_steps':
        assert ran is None, f'{case.id}: meant for k_small_steps, ran k_step2'
    else:
        assert ran == V.expected_kernel(case, before), f'{case.id}: meant for k_step2 {V.expected_kernel(case, before)}, ran {ran}'
    return (entries[0] if entries else None), ran


@pytest.fixture(scope='module')
def handles():
    """The sweeps' Problems, one per (test, case), shared by the parts of a sweep and released with the module."""
    cache = {}
    yield cache
    cache.clear()


def handle(handles, key, case):
    """The Problem of `key`, made on first use (call inside environment(V.env_of(case)))."""
    if key not in handles:
        from gapflow_amd import Problem
        gpu = V.make(Problem, case)
        np.testing.assert_array_equal(gpu.q, V.base_state(case))
        handles[key] = gpu
    return handles[key]


def parts_of(case):
    return 3 if case.nx * case.ny > 4000 else 1


def sweep_params(cases):
    return [pytest.param(c, k, id=c.id + (f'-part{k}' if parts_of(c) > 1 else '')) for c in cases for k in range(parts_of(c))]


def set_state(gpu, q):
    gpu.q[...] = q


def sweeps(gpu, case, jobs, steps_per_job, body):
    """body(job) for every job, twice; between the two sweeps as many unplanted steps as it takes for every job to meet the other
    predictor direction (MC_order 0: the direction alternates with the step index)."""
    seen = {}
    for sweep in range(2):
        for k, job in enumerate(jobs):
            seen.setdefault(k, set()).add(gpu.step % 2)
            body(job)
        if sweep == 0:
            for _ in range(1 + (len(jobs) * steps_per_job) % 2):
                set_state(gpu, V.base_state(case))
                rec, _ = take_step(gpu, case)
                assert rec is not None and rec.invalid == 0
    assert all(s == {0, 1} for s in seen.values()), 'a position met one predictor direction only'


def max_jobs(case):
    jobs = [('spike', p) for p in V.interior(case)]
    if case.bc == 'dd':
        jobs += [(kind, p) for kind in ('below', 'above') for p in V.edge_cells(case)]
    return jobs


# ---- 1: planted maximum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,part', sweep_params(V.MAX_CASES))
def test_planted_maximum_reaches_the_record(hiplib, handles, case, part):
    worst = np.zeros(3)
    ran = set()

    def body(job):
        kind, pos = job
        set_state(gpu, V.plant(case, kind, pos))
        rec, kernel = take_step(gpu, case)
        ran.add(kernel)
        assert rec is not None and rec.invalid == 0, f'{case.id}: {kind} at {pos}: the step was refused'
        ekin, v_max, v_sound, at = V.reference_scalars(gpu.q, case.law)
        assert at in V.images_of(case, pos), f'{case.id}: {kind} at {pos}: the maximum sits at {at}'
        if kind == 'above':
            assert at != pos, f'{case.id}: above at {pos}: the interior cell holds the maximum'
        err = np.abs(np.array([rec.ekin / ekin, rec.v_max / v_max, rec.v_sound / v_sound]) - 1.)
        worst[...] = np.maximum(worst, err)
        what = f'{case.id}: {kind} at {pos}, D {1 if (rec.step - 1) % 2 == 0 else -1}'
        np.testing.assert_allclose(rec.v_max, v_max, rtol=VMAX_RTOL, err_msg=what)
        np.testing.assert_allclose(rec.ekin, ekin, rtol=EKIN_RTOL, err_msg=what)
        np.testing.assert_allclose(rec.v_sound, v_sound, rtol=VSOUND_RTOL, err_msg=what)

    jobs = max_jobs(case)[part::parts_of(case)]
    try:
        with environment(V.env_of(case)):
            gpu = handle(handles, ('maximum', case.id), case)
            sweeps(gpu, case, jobs, 1, body)
    except BaseException:
        handles.pop(('maximum', case.id), None)        # a halted handle is not handed to the next part
        raise
    finally:
        if part == parts_of(case) - 1:
            handles.pop(('maximum', case.id), None)     # the last part of the sweep: release the handle
        print(f'\n[{case.id}] planted maximum: {len(jobs)} positions x 2 directions, ran {sorted(map(str, ran))}; worst relative error of '
              f'(ekin, v_max, v_sound) {worst} (tolerance {EKIN_RTOL:g}, {VMAX_RTOL:g}, {VSOUND_RTOL:g})')


# ---- 2: planted imaginary sound speed --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,part', sweep_params(V.SOUND_CASES))
def test_planted_imaginary_sound_speed_reaches_the_record(hiplib, handles, case, part):
    ran = set()

    def body(job):
        kind, pos = job
        set_state(gpu, V.plant(case, kind, pos))
        step = gpu.step
        rec, kernel = take_step(gpu, case)
        ran.add(kernel)
        what = f'{case.id}: {kind} at {pos}, D {1 if step % 2 == 0 else -1}'
        assert rec is not None and rec.invalid == 0 and rec.step == step + 1, f'{what}: the step did not commit'
        assert np.isnan(rec.v_sound), f'{what}: v_sound {rec.v_sound!r}'
        set_state(gpu, V.base_state(case))
        rec, _ = take_step(gpu, case)
        assert rec is not None and rec.invalid == 0 and rec.step == step + 2, f'{what}: the next step did not commit'
        assert np.isfinite(rec.v_sound) and rec.v_sound > 0., f'{what}: v_sound of the next, unplanted step {rec.v_sound!r}'

    jobs = [('spinodal', p) for p in V.interior(case)]
    if case.bc == 'dd':
        jobs += [('image', p) for p in V.edge_cells(case)]
    jobs = jobs[part::parts_of(case)]
    try:
        with environment(V.env_of(case)):
            gpu = handle(handles, ('sound', case.id), case)
            set_state(gpu, V.base_state(case))          # the control: nothing planted, a real sound speed
            rec, _ = take_step(gpu, case)
            ref = V.sound_speed(case.law, np.array(gpu.q[0])).max()
            assert rec is not None and np.isfinite(ref)
            np.testing.assert_allclose(rec.v_sound, ref, rtol=VSOUND_RTOL, err_msg=f'{case.id}: nothing planted')
            sweeps(gpu, case, jobs, 2, body)
    except BaseException:
        handles.pop(('sound', case.id), None)
        raise
    finally:
        if part == parts_of(case) - 1:
            handles.pop(('sound', case.id), None)
        print(f'\n[{case.id}] planted imaginary sound speed: {len(jobs)} positions x 2 directions, ran {sorted(map(str, ran))}')


# ---- 3 and 4: planted NaN, negative density, zero density ------------------------------------------------------------------------
def invalid_jobs(case):
    """(label, planted q, the interior cells planted) of parts 3 and 4."""
    jobs = []
    for pos in V.invalid_positions(case):
        for kind in ('nan-rho', 'nan-jx', 'nan-jy', 'negative', 'zero'):
            jobs.append((f'{kind} at {pos}', V.plant(case, kind, pos), [pos]))
    if case.path != 'k_small_steps':
        for pos in V.row_sweep(case):
            for kind in V.ROW_SWEEP_KINDS[::1 if pos[0] % 2 else -1]:       # (each kind meets both predictor directions down the rows)
                jobs.append((f'{kind} at {pos}', V.plant(case, kind, pos), [pos]))
    if case.bc == 'dd':
        nx, ny = case.nx, case.ny
        for pos in {(1, (ny + 1) // 2), (nx, (ny + 1) // 2), ((nx + 1) // 2, 1), ((nx + 1) // 2, ny)}:
            jobs.append((f'ghost-negative at {pos}', V.plant(case, 'ghost-negative', pos), [pos]))
    a, b = V.far_pair(case)
    if a != b:
        for first, second in ((a, b), (b, a)):
            jobs.append((f'nan-jy at {first} and negative at {second}', V.plant(case, 'negative', second, V.plant(case, 'nan-jy', first)),
                         [first, second]))
    return jobs


def check_refusal(what, case, gpu, q, cells, want, step_before):
    """A refused (or, should the oracle commit it, a committed) step of `gpu` against the oracle's outcome `want`."""
    from gapflow_amd import _lib
    sc = gpu._scalars()
    assert want['stopped'] == (sc.invalid != 0), f'{what}: the oracle {"stops" if want["stopped"] else "commits"}, invalid = {sc.invalid}'
    assert sc.invalid == want['invalid'], f'{what}: invalid {sc.invalid}, the oracle {want["invalid"]}'
    assert sc.step == step_before + (0 if want['stopped'] else 1), f'{what}: step {sc.step}'
    if not want['stopped']:
        return
    got = gpu._download(_lib.FIELD_Q, 3)
    np.testing.assert_array_equal(got, q, err_msg=f'{what}: q behind the refused step')
    np.testing.assert_array_equal(want['q'], q)
    _lib.check(gpu._lib.gpf_update_closures(gpu._h))
    p = gpu._download(_lib.FIELD_PRESSURE, 1)[0]
    clean = np.ones(p.shape, bool)
    for pos in cells:
        for c in V.images_of(case, pos):
            clean[c] = False
    scale = np.abs(want['pressure'][clean]).max()
    err = np.abs(p - want['pressure'])[clean].max()
    assert err <= PRESSURE_TOL * scale, f'{what}: pressure behind the refused step {err / scale:.1e} of scale away from the oracle'


@pytest.mark.parametrize('case', V.INVALID_CASES, ids=[c.id for c in V.INVALID_CASES])
def test_planted_invalid_cell_stops_the_run(hiplib, case):
    from gapflow_amd import Problem
    ran, counts, spread = set(), {}, set()
    jobs = invalid_jobs(case)
    try:
        with environment(V.env_of(case)):
            for k, (label, q, cells) in enumerate(jobs):
                steps_before = k % 2                        # both predictor directions down the list
                want = V.oracle_outcome(case, q, steps_before)
                gpu = V.make(Problem, case)
                for _ in range(steps_before):
                    rec, _ = take_step(gpu, case)
                    assert rec is not None
                set_state(gpu, q)
                rec, kernel = take_step(gpu, case)
                ran.add(kernel)
                assert (rec is None) == want['stopped'], f'{case.id}: {label}: the oracle {"stops" if want["stopped"] else "commits"}'
                if len(cells) == 2 and case.path in ('k_step2', 'split'):       # the two flags come from different blocks (waves, where
                    note = gpu._lib.gpf_plan_note(gpu._h).decode()              # the plan has one block only), by the plan in force
                    nchunks = int(note.split(' chunks per strip')[0])
                    assert not case.chunks or nchunks == case.chunks, note
                    (b0, w0), (b1, w1) = (V.wave_of(case, nchunks, c, 1 if steps_before % 2 == 0 else -1) for c in cells)
                    spread.add((abs(w1 - w0) + 1, abs(b1 - b0) + 1))
                    assert w0 != w1 and (b0 != b1 or max(w0, w1) < 4), f'{case.id}: {label}: waves {w0}, {w1} of blocks {b0}, {b1} ({note})'
                check_refusal(f'{case.id}: {label}', case, gpu, q, cells, want, steps_before)
                counts[want['invalid']] = counts.get(want['invalid'], 0) + 1
    finally:
        print(f'\n[{case.id}] planted invalid cells: {len(jobs)} cases, each under one predictor direction (alternating down the list), outcomes '
              f'{counts} (invalid: count), ran {sorted(map(str, ran))}' + (f'; the two-flag cases span (waves, blocks) {sorted(spread)}' if spread else ''))


# ---- ensembles -------------------------------------------------------------------------------------------------------------------
def ensemble_members(case):
    """Thirty planted members chosen by construction: every kind of part 3 and the zero cell, each at the four corners in turn and
    at the middle; the ghost-only negative density on each of the four edges; a NaN and a negative density in one member."""
    nx, ny = case.nx, case.ny
    mx, my = (nx + 1) // 2, (ny + 1) // 2
    corners = [(1, 1), (nx, ny), (1, ny), (nx, 1)]
    out = []
    for k, kind in enumerate(('nan-rho', 'nan-jx', 'nan-jy', 'negative', 'zero')):
        for pos in (corners[k % 4], corners[(k + 1) % 4], (mx, my), (nx, my), (mx, ny)):
            out.append((f'{kind} at {pos}', V.plant(case, kind, pos), [pos]))
    for pos in ((1, my), (nx, my), (mx, 1), (mx, ny)):
        out.append((f'ghost-negative at {pos}', V.plant(case, 'ghost-negative', pos), [pos]))
    a, b = V.far_pair(case)
    out.append((f'nan-jy at {a} and negative at {b}', V.plant(case, 'negative', b, V.plant(case, 'nan-jy', a)), [a, b]))
    return out


@pytest.mark.parametrize('tier', ['lds', 'workspace'])
def test_ensemble_members_decide_alone(hiplib, tier):
    """k_small_ensemble (9 x 20, planes in LDS) and k_mid_ensemble (37 x 40, forced): every other member carries its own planted
    cell, the members between them none; each invalid member's outcome is the oracle's for its own state, each valid member's
    field and record are bit for bit its solo run's: the same member as the only one of an ensemble of the same tier."""
    from gapflow_amd import Ensemble, Problem, _lib
    shape = V.ENSEMBLE_SHAPES[tier]
    case = V._case('DH', 'planes', shape, 'dd', 'ensemble')
    planted = ensemble_members(case)
    force = 'workspace' if tier == 'workspace' else 'auto'

    def members(states):
        ps = [V.make(Problem, case) for _ in states]
        for p, q in zip(ps, states):
            if q is not None:
                p.q[...] = q
        ens = Ensemble(ps, tier=force)
        assert ens.tiers == [tier] * len(ps)
        ens.step(1)
        return ps

    states = [s for job in planted for s in (job[1], None)]
    assert len(states) <= 64
    ps = members(states)
    solo = members([None])[0]
    q_solo, sc_solo = solo._download(_lib.FIELD_Q, 3), solo._scalars()
    assert sc_solo.step == 1 and sc_solo.invalid == 0 and step_variant(solo) is None
    for i, p in enumerate(ps):
        assert step_variant(p) is None
        if states[i] is None:
            sc = p._scalars()
            assert sc.step == 1 and sc.invalid == 0, f'member {i} (valid) next to {planted[(i - 1) // 2][0]}: step {sc.step}, invalid {sc.invalid}'
            np.testing.assert_array_equal(p._download(_lib.FIELD_Q, 3), q_solo, err_msg=f'member {i} (valid)')
            assert (sc.ekin, sc.v_max, sc.v_sound) == (sc_solo.ekin, sc_solo.v_max, sc_solo.v_sound)
        else:
            label, q, cells = planted[i // 2]
            check_refusal(f'{tier} ensemble, member {i}: {label}', case, p, q, cells, V.oracle_outcome(case, q), 0)
    print(f'\n[{tier} ensemble {shape[0]} x {shape[1]}] {len(planted)} planted members between {len(planted)} valid ones, '
          f'ran {"k_small_ensemble" if tier == "lds" else "k_mid_ensemble"}')


# ---- slabs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('part', range(3))
def test_three_slabs_stop_together(hiplib, part):
    """Three x-slabs as threads (13 + 12 + 12 rows of 37 x 40, the all-gather transport): a cell planted in each rank in turn, on a
    seam row and away from it.  Every rank stops at the step the oracle stops at, with the oracle's `invalid`, and holds its rows
    of the planted q bit for bit, outer rows included."""
    import torch
    from gapflow_amd import _lib
    from gapflow_amd.slab import SlabProblem, ThreadWorld, partition
    case = V.SLAB_CASE
    assert (case.nx, case.ny) == __import__('edge_rule_cases').SLAB_SHAPE
    text = V.case_text(case)
    base = V.base_state(case)
    bounds = [tuple(b) for b in partition(case.nx, V.SLAB_RANKS)]
    jobs = V.slab_jobs(case, bounds)[part::3]          # (a third of the cases per test: each builds three slabs anew)
    wants = [V.oracle_outcome(case, q, k % 2) for k, (_, q, _) in enumerate(jobs)]

    def rank_body(group):
        out = []
        for k, (label, q, cells) in enumerate(jobs):
            slab = SlabProblem.from_string(text, device=0, dist=group)
            slab.pre_run()
            L = slab.layout
            assert (L.lo, L.hi) == bounds[L.rank]
            rows = slice(L.lo - 1, L.hi + 2)
            slab._upload(_lib.FIELD_Q, base[:, rows])
            _lib.check(slab.lib.gpf_set_ekin_old(slab._h, float(slab.global_scalars()['ekin'])))
            slab.advance(k % 2)                             # both predictor directions down the list
            before = int(slab.state().step)
            slab._upload(_lib.FIELD_Q, q[:, rows])
            slab.advance(1)
            st = slab.state()
            variant = (C.c_int * 5)()
            ran = tuple(variant) if slab.lib.gpf_step_variant(slab._h, variant) == 0 else None
            out.append((L.rank, before, int(st.step), int(st.invalid), slab.local_q(), rows, ran))
        return out

    runs = ThreadWorld(V.SLAB_RANKS, torch).run(rank_body)
    assert len(runs) == V.SLAB_RANKS
    counts = {}
    for k, (label, q, cells) in enumerate(jobs):
        want = wants[k]
        assert want['stopped'], label
        for rank, before, step, invalid, got, rows, ran in (r[k] for r in runs):
            what = f'slab {rank} of {V.SLAB_RANKS}: {label}'
            assert ran == V.expected_kernel(case, k % 2), f'{what}: ran {ran}'
            assert before == k % 2 and step == before, f'{what}: step {step} after {before}'
            assert invalid == want['invalid'], f'{what}: invalid {invalid}, the oracle {want["invalid"]}'
            np.testing.assert_array_equal(got, q[:, rows], err_msg=f'{what}: rows behind the refused step')
        counts[want['invalid']] = counts.get(want['invalid'], 0) + 1
    print(f'\n[slabs {case.nx} x {case.ny}, rows {bounds}] {len(jobs)} planted cases, each under one predictor direction, outcomes {counts} '
          f'(invalid: count), ran k_step2 {V.expected_kernel(case, 0)} and {V.expected_kernel(case, 1)} on every rank')
