"""options.integrals / options.integrals_sections_x / _y: read from the YAML text beside the sanitised dictionaries and checked on
the host, and the slot arithmetic of a recording batch -- no GPU and no library call (the device side: tests/test_gpu_integrals.py)."""
import io

import numpy as np
import pytest

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_integrals
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_integrals(d, text)
    return d, before


def test_integrals_keys_are_read_from_the_yaml_text():
    d, _ = parsed(", integrals: 5, integrals_sections_x: [1, 50, 100], integrals_sections_y: [3]")
    assert d['options']['integrals'] == 5
    assert d['options']['integrals_sections_x'] == [1, 50, 100] and d['options']['integrals_sections_y'] == [3]
    d, _ = parsed(", integrals: 1")
    assert d['options']['integrals'] == 1 and 'integrals_sections_x' not in d['options'] and 'integrals_sections_y' not in d['options']


def test_absent_key_leaves_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and not any(k.startswith('integrals') for k in d['options'])
    d, before = parsed(", integrals_sections_x: [1, 2]")        # means nothing without the stride
    assert d == before


@pytest.mark.parametrize('bad', ["0", "-3", "1.5", "True", "[1]", "'often'"])
def test_malformed_stride_raises(bad):
    with pytest.raises(ValueError, match='integrals'):
        parsed(f", integrals: {bad}")


@pytest.mark.parametrize('bad', ["[]", "7", "[0]", "[101]", "[1.5]", "[True]", "['a']", "{a: 1}", "[[1, 2]]", "[-1]",
                                 "[1, 2, 3, 4, 5, 6, 7, 8, 9]"])
def test_malformed_or_out_of_range_sections_raise(bad):
    with pytest.raises(ValueError, match='integrals_sections_x'):
        parsed(f", integrals: 2, integrals_sections_x: {bad}")
    if bad != "[1, 2, 3, 4, 5, 6, 7, 8, 9]":
        with pytest.raises(ValueError, match='integrals_sections_y'):
            parsed(f", integrals: 2, integrals_sections_y: {bad.replace('101', '7')}")


def test_section_validation_and_defaults_on_the_host():
    from gapflow_amd.problem import _integral_sections
    assert _integral_sections(None, 100, 'sections_x') == [1, 100]
    assert _integral_sections(None, 1, 'sections_y') == [1]            # a direction of extent 1 has the one section
    assert _integral_sections(np.array([3, 1, 3]), 4, 'sections_x') == [3, 1, 3]
    assert _integral_sections((1, 2, 3, 4, 5, 6, 7, 8), 8, 'sections_x') == list(range(1, 9))
    with pytest.raises(ValueError, match=r'sections_y\[1\] = 7 lies outside the interior 1\.\.6'):
        _integral_sections([1, 7], 6, 'sections_y')
    with pytest.raises(ValueError, match='9 sections'):
        _integral_sections([1] * 9, 100, 'sections_x')


@pytest.mark.parametrize('every', [1, 2, 3, 7, 50, 4096])
def test_slot_arithmetic_against_a_brute_force_count(every):
    from gapflow_amd.problem import _integral_records
    for base in (0, 1, 6, 7, 8, 49, 50, 4095, 4096, 12345):
        for ran in (0, 1, 2, 6, 7, 8, 13, 14, 50, 99, 4096):
            brute = sum(1 for s in range(base + 1, base + ran + 1) if s % every == 0)
            assert _integral_records(base, ran, every) == brute, (base, ran, every)
        # the slot of a recorded step is its rank among the batch's recorded steps
        recorded = [s for s in range(base + 1, base + 200) if s % every == 0]
        for rank, s in enumerate(recorded):
            assert _integral_records(base, s - base, every) - 1 == rank


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='integrals: not available on a SlabProblem'):
        SlabProblem.set_integrals(object(), every=2)
    with pytest.raises(NotImplementedError, match='integrals: not available on a SlabProblem'):
        SlabProblem.film_integrals(object())
    with pytest.raises(NotImplementedError, match='integrals: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", integrals: 4"), device=0, dist=object())


def test_film_pressure_stays_in_step_with_eos_pressure(tmp_path):
    """closures.hpp holds Dowson-Higginson twice: eos_pressure<EOS_DH> (s = rho * (1 / rho0), reciprocals) for the step kernels,
    the derived fields and the probes, film_pressure<EOS_DH> (the reference's divisions) for the load.  Same source compiled for
    the host, under the sanitizers: film_pressure equals oracle/closures.py in every bit (the same IEEE operations in the same
    order), and the two stay within the rounding that separates them, so neither clamp nor formula can change in one alone.
    With u = 2^-53: the two s differ by at most 3 u s (one rounding against two), which the law turns into
    3 u s C1 (C2 - 1) / (C2 - s)^2 -- 4 u here, for the second-order term, at most 3 u s / (C2 - s) <= 3e-14 of the first under the
    clamp at 0.99 C2; the quotient C1 (s - 1) / (C2 - s) takes 4 roundings in one form and 5 in the other, 10 u |p - P0| with one
    to spare; the final sums one each, 2 u |p|."""
    import os
    import shutil
    import subprocess
    from oracle import closures as ocl
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / 'film_pressure_host')
    res = subprocess.run([shutil.which('g++'), '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                          '-fno-sanitize-recover=all', '-Wall', '-Werror', os.path.join(here, 'hostcheck', 'film_pressure_host.cpp'), '-o', exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    u = 2.0 ** -53
    rng = np.random.default_rng(11)
    for rho0, P0, C1, C2 in ((877.7007, 101325., 3.5e10, 1.23), (877.7007, 1.e8, 3.5e8, 1.23), (850., 1.e5, 2.2e9, 1.66)):
        cap = 0.99 * C2 * rho0
        rho = np.concatenate([rho0 * (1. + np.linspace(-0.1, 5.e-4, 3001)), rho0 * (1. + rng.uniform(-1.e-3, 1.e-3, 3000)),
                              np.linspace(rho0, 1.05 * cap, 2001), [rho0, cap, np.nextafter(cap, 0.), np.nextafter(cap, 2. * cap), 2. * cap]])
        data = np.concatenate([[float(rho.size)], [rho0, P0, C1, C2, 0., 0., 0., 0.], rho])
        res = subprocess.run([exe], input=data.tobytes(), capture_output=True,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
        assert res.returncode == 0 and res.stderr == b'', res.stderr.decode()[-3000:]
        out = np.frombuffer(res.stdout, dtype=float)
        assert out.size == 2 * rho.size
        eos, film = out[:rho.size], out[rho.size:]
        ref = ocl.eos_pressure(rho, dict(EOS='DH', rho0=rho0, P0=P0, C1=C1, C2=C2))
        assert film.tobytes() == ref.tobytes(), f"film_pressure against the oracle: {np.abs(film - ref).max():.3e}"
        s = np.minimum(rho, cap) / rho0
        tol = 4. * u * s * C1 * (C2 - 1.) / (C2 - s) ** 2 + 10. * u * np.abs(ref - P0) + 2. * u * np.abs(ref)
        worst = np.argmax(np.abs(eos - film) / tol)
        print(f"\n[DH C1 {C1:g} P0 {P0:g}] largest |eos_pressure - film_pressure| / bound {np.abs(eos - film)[worst] / tol[worst]:.3f} at rho / rho0 = "
              f"{rho[worst] / rho0:.6f}; largest relative difference {np.max(np.abs(eos - film) / np.abs(ref)):.2e}")
        assert np.all(np.abs(eos - film) <= tol), f"rho = {rho[worst]!r}: eos_pressure {eos[worst]!r}, film_pressure {film[worst]!r}, bound {tol[worst]:.3e}"
        assert np.abs(eos - film).max() > 0.        # the two forms do differ: the case the bound is about
