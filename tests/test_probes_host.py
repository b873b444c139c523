"""options.probes / options.probes_pressure: read from the YAML text beside the sanitised dictionaries and checked on the host --
no GPU and no library call (the device side: tests/test_gpu_probes.py)."""
import io

import numpy as np
import pytest

BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 1, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_probes
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    before = {k: dict(v) if isinstance(v, dict) else v for k, v in d.items()}
    _keep_probes(d, text)
    return d, before


def test_probes_key_is_read_from_the_yaml_text():
    d, _ = parsed(", probes: [[0, 1], [50, 1], [101, 2]], probes_pressure: False")
    assert d['options']['probes'] == [[0, 1], [50, 1], [101, 2]]
    assert d['options']['probes_pressure'] is False
    d, _ = parsed(", probes: [[7, 0]]")
    assert d['options']['probes'] == [[7, 0]] and 'probes_pressure' not in d['options']


def test_absent_key_leaves_the_dictionaries_unchanged():
    d, before = parsed("")
    assert d == before and 'probes' not in d['options'] and 'probes_pressure' not in d['options']
    d, before = parsed(", probes_pressure: True")           # means nothing without probes
    assert d == before


@pytest.mark.parametrize('bad', ["[[1]]", "[[1, 2, 3]]", "[1, 2]", "[[1.5, 1]]", "[['a', 1]]", "[]", "7", "[[True, 1]]", "{a: 1}",
                                 "[[102, 1]]", "[[1, 3]]", "[[-1, 1]]"])
def test_malformed_entries_raise(bad):
    with pytest.raises(ValueError, match='probes'):
        parsed(f", probes: {bad}")


def test_cell_validation_on_the_host():
    from gapflow_amd.problem import _probe_cells
    cells = _probe_cells([(0, 0), (101, 2), np.array([3, 1])], (102, 3))
    assert cells.tolist() == [[0, 0], [101, 2], [3, 1]] and cells.shape == (3, 2)
    assert _probe_cells(np.array([[5, 1], [6, 1]]), (102, 3)).tolist() == [[5, 1], [6, 1]]
    with pytest.raises(ValueError, match=r'\(102, 1\) \(entry 1\)'):
        _probe_cells([(1, 1), (102, 1)], (102, 3))
    with pytest.raises(ValueError, match='257'):
        _probe_cells([(1, 1)] * 257, (102, 3))
    assert len(_probe_cells([(1, 1)] * 256, (102, 3))) == 256


def test_slab_problem_refuses_before_it_touches_a_device():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='probes: not available on a SlabProblem'):
        SlabProblem.set_probes(object(), [(1, 1)])
