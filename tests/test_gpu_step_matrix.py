"""Every instantiation of k_step2 (csrc/step2_kernel.hip: <EOS, HAS_LS, PIEZO, D, TOPO>) that step2_kernel() (csrc/api.hip) can
select, against the oracle: seven equations of state x eight variants x both sweep directions (tests/step_matrix_cases.py), TOPO 1
with a dh/dy that is not zero, and long marches of the heavy laws.  Six steps each; q with its ghost cells and corners per
component at the project's tolerance (helpers.field_tol on the oracle's own one-ulp response), the scalars, the stress field of the
piezo-viscous cases -- and gpf_step_variant's record of what each step launched, so that a case cannot pass on another kernel."""
import ctypes as C

import numpy as np
import pytest

from helpers import comp_err, field_tol, HISTORY_RTOL
from step_matrix_cases import CASES, IDS, LAWS, EOS_ID, EXPECTED, STEPS, env_of, environment, make, oracle_run

pytestmark = pytest.mark.gpu


def kernel_name(v):
    law = {i: n for n, i in EOS_ID.items()}.get(v[0], v[0])
    return f'k_step2<{law}, HAS_LS {v[1]}, PIEZO {v[2]}, D {v[3]:+d}, TOPO {v[4]}>'


def step_variant(prob):
    from gapflow_amd import _lib
    out = (C.c_int * 5)()
    _lib.check(prob._lib.gpf_step_variant(prob._h, out))
    return tuple(out)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_step_matches_oracle(hiplib, case):
    from gapflow_amd import Problem
    ref = oracle_run(case)
    has_ls, piezo, topo = EXPECTED[case.variant]
    with environment(env_of(case)):
        gpu = make(Problem, case)
        np.testing.assert_array_equal(gpu.q, ref['q0'])
        launched = []
        for _ in range(STEPS):
            gpu.update()
            launched.append(step_variant(gpu))
        note = gpu._lib.gpf_plan_note(gpu._h).decode()
        q, dt, ekin, mass, v_sound = gpu.q.copy(), gpu.dt, gpu.kinetic_energy, gpu.mass, gpu.pressure.v_sound
        stress = np.array(gpu.bulk_stress.stress) if piezo else None
    # MC_order 0: D = +1 in the even steps, -1 in the odd ones
    expected = [(EOS_ID[case.law], has_ls, piezo, 1 if s % 2 == 0 else -1, topo) for s in range(STEPS)]
    for s, (got, want) in enumerate(zip(launched, expected)):
        assert got == want, f'{case.id}, step {s}: meant for {kernel_name(want)}, ran {kernel_name(got)}'
    names = ' and '.join(kernel_name(v) for v in expected[:2])
    assert note, f'{names}: k_step2 was never planned'
    if topo >= 3:
        assert ('row coefficients from the table' if topo == 4 else 'row coefficients evaluated in the kernel') in note, note
    if case.chunks:
        assert note.startswith(f'{case.chunks} chunks per strip'), note
    assert gpu.step == ref['steps'] == STEPS
    tol = field_tol({'sens_end': ref['sens']}, 'end')
    err = comp_err(q, ref['q'])
    print(f'\n[{case.id}] {names}: error of (rho, jx, jy) {err} of scale, tolerance {tol}; relative error of dt {abs(dt / ref["dt"] - 1):.1e}, '
          f'ekin {abs(ekin / ref["ekin"] - 1):.1e}, mass {abs(mass / ref["mass"] - 1):.1e}, v_sound {abs(v_sound / ref["v_sound"] - 1):.1e}')
    assert (err <= tol).all(), f'{names}: q after {STEPS} steps: error {err}, tolerance {tol}'
    np.testing.assert_allclose(dt, ref['dt'], rtol=1e-9, err_msg=names)
    np.testing.assert_allclose(ekin, ref['ekin'], rtol=1e-9, err_msg=names)
    np.testing.assert_allclose(mass, ref['mass'], rtol=1e-12, err_msg=names)
    np.testing.assert_allclose(v_sound, ref['v_sound'], rtol=1e-9 if LAWS[case.law].pow_exp else HISTORY_RTOL[5], err_msg=names)
    if piezo:       # the stress field as update() leaves it: the corrector stage's closure, as test_piezoviscosity_steps_match_oracle
        np.testing.assert_allclose(stress, ref['tau_avg'], rtol=1e-9, atol=1e-9 * np.abs(ref['tau_avg']).max(), err_msg=names)


def test_matrix_ran_every_instantiation():
    """The expected tuples of the table, which every case above asserts step by step: all 56 (law, variant) pairs, both D."""
    seen = {(EOS_ID[c.law],) + EXPECTED[c.variant] for c in CASES}
    assert seen == {(e, ls, pz, topo) for e in range(7) for ls, pz, topo in set(EXPECTED.values())} and len(seen) == 56
    assert STEPS >= 2           # an even and an odd step
