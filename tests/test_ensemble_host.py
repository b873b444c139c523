"""Host side of the ensembles (gapflow_amd/ensemble.py, __main__): no GPU, no library call."""
import pytest

BASE = {'options': {'silent': True}, 'grid': {'Nx': 100, 'Ny': 1, 'dx': 1.e-5, 'dy': 1.},
        'geometry': {'type': 'journal', 'CR': 1.e-2, 'eps': 0.7, 'U': 0.1, 'V': 0.},
        'numerics': {'CFL': 0.25, 'adaptive': 1, 'tol': 1.e-8, 'max_it': 100},
        'properties': {'EOS': 'DH', 'shear': 0.0794, 'bulk': 0., 'rho0': 877.7007, 'piezo': {'name': 'Barus', 'aB': 2.e-8}}}


def test_sweep_order_and_parameters():
    """The Cartesian product in itertools.product order: the first axis slowest, the last fastest; `parameters` says who got what."""
    from gapflow_amd.ensemble import sweep_members
    dicts, params = sweep_members(BASE, {'geometry.eps': [0.5, 0.7, 0.9], 'geometry.U': [0.1, 0.2], 'properties.piezo.aB': [1.e-8]})
    assert len(dicts) == len(params) == 6
    assert [(p['geometry.eps'], p['geometry.U']) for p in params] == [(0.5, 0.1), (0.5, 0.2), (0.7, 0.1), (0.7, 0.2), (0.9, 0.1), (0.9, 0.2)]
    for d, p in zip(dicts, params):
        assert d['geometry']['eps'] == p['geometry.eps'] and d['geometry']['U'] == p['geometry.U']
        assert d['properties']['piezo']['aB'] == 1.e-8 and d['properties']['piezo']['name'] == 'Barus'
        assert d['grid'] == BASE['grid'] and d['grid'] is not BASE['grid']
    assert BASE['geometry']['eps'] == 0.7 and BASE['properties']['piezo']['aB'] == 2.e-8        # the input is not edited


def test_sweep_takes_numpy_values():
    import numpy as np
    import yaml
    from gapflow_amd.ensemble import sweep_members
    dicts, params = sweep_members(BASE, {'geometry.U': np.linspace(0.1, 0.3, 3)})
    assert len(dicts) == 3 and [d['geometry']['U'] for d in dicts] == [float(v) for v in np.linspace(0.1, 0.3, 3)]
    assert all(type(d['geometry']['U']) is float for d in dicts)
    assert yaml.full_load(yaml.safe_dump(dicts[1]))['geometry']['U'] == dicts[1]['geometry']['U']       # survives the YAML text


@pytest.mark.parametrize('key', ['geometri.eps', 'geometry.epsilon', 'eps', 'properties.piezo.z', 'geometry.eps.x'])
def test_sweep_bad_key_raises_keyerror(key, monkeypatch):
    """... before any device work: no Problem is built."""
    from gapflow_amd import Ensemble, Problem
    from gapflow_amd.ensemble import sweep_members
    with pytest.raises(KeyError):
        sweep_members(BASE, {'geometry.U': [0.1, 0.2], key: [1., 2.]})
    import yaml
    monkeypatch.setattr(Problem, 'from_string', classmethod(lambda cls, *a, **k: pytest.fail("a Problem was built")))
    with pytest.raises(KeyError):
        Ensemble.sweep(yaml.safe_dump(BASE), {key: [1., 2.]})


def test_sweep_needs_values():
    from gapflow_amd.ensemble import sweep_members
    with pytest.raises(ValueError):
        sweep_members(BASE, {})
    with pytest.raises(ValueError):
        sweep_members(BASE, {'geometry.eps': []})


def test_empty_ensemble_is_refused_on_the_host():
    from gapflow_amd import Ensemble
    with pytest.raises(ValueError, match="at least one member"):
        Ensemble([])
    with pytest.raises(TypeError, match="member 0"):
        Ensemble(["journal.yaml"])


def test_batch_length_rule():
    """The shared helper is the rule Problem.run used inline: steps to the next frame, to max_it, to the next checkpoint, at
    most 4096 -- restated here term by term."""
    from gapflow_amd.problem import _batch_length
    for step, wf, max_it, cf in [(0, 1000, 100000, 0), (0, 10000, 100000, 0), (999, 1000, 100000, 0), (1000, 1000, 1003, 0),
                                 (30, 25, 35, 10), (7, 25, 1000, 10), (4090, 5000, 9000, 4096), (0, 1, 5, 0), (12, 5000, 100000, 7)]:
        want = min(wf - step % wf, max_it - step, 4096, *([cf - step % cf] if cf > 0 else []))
        assert _batch_length(step, wf, max_it, cf) == want, (step, wf, max_it, cf)
        assert 1 <= want <= 4096
    assert _batch_length(0, 10000, 100000) == 4096


def test_problem_run_uses_the_shared_rule():
    """Problem._run_batch_length is the helper on the problem's own step, write_freq and max_it (no device: a bare object)."""
    from gapflow_amd import Problem
    from gapflow_amd.problem import _batch_length
    p = Problem.__new__(Problem)
    p.step, p.max_it, p.options = 30, 35, {'write_freq': 25, 'silent': False}
    assert p._run_batch_length(10) == _batch_length(30, 25, 35, 10) == 5
    assert p._run_batch_length(0) == 5
    p.step, p.max_it = 0, 100000
    assert p._run_batch_length(0) == 25


def test_main_with_one_input_takes_the_old_path(monkeypatch):
    """One -i file: Problem.from_yaml(...).run(), as ever; Ensemble is not touched.  Several: Ensemble.from_yaml with all of them."""
    import gapflow_amd.__main__ as cli
    import gapflow_amd.ensemble as ens
    calls = []

    class Stub:
        def __init__(self, what):
            self.what = what

        def run(self):
            calls.append(('run', self.what))

    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(cli.Problem, 'from_yaml', classmethod(lambda cls, f, device=0: calls.append(('problem', f, device)) or Stub('problem')))
    monkeypatch.setattr(ens.Ensemble, 'from_yaml', classmethod(lambda cls, fs, device=0: calls.append(('ensemble', list(fs), device)) or Stub('ensemble')))
    assert cli.main(['-i', 'a.yaml', '--device', '0']) == 0
    assert calls == [('problem', 'a.yaml', 0), ('run', 'problem')]
    del calls[:]
    assert cli.main(['-i', 'a.yaml', 'b.yaml', 'c.yaml']) == 0
    assert calls == [('ensemble', ['a.yaml', 'b.yaml', 'c.yaml'], 0), ('run', 'ensemble')]
    o = cli.make_parser().parse_args(['-i', 'input.yaml'])
    assert o.filename == 'input.yaml' and o.restart is None


def test_small_grid_switch_reads_like_atoi():
    """The host mirror of GPF_SMALL_GRID follows the library's atoi: anything without leading digits is 0, which is off."""
    from gapflow_amd.ensemble import _atoi
    assert [_atoi(t) for t in ('0', '1', ' 0', '-0', 'off', '', '0x1', '2 ', '+3', 'no0')] == [0, 1, 0, 0, 0, 0, 0, 2, 3, 0]


def test_sweep_takes_a_path_object(tmp_path, monkeypatch):
    import yaml
    from gapflow_amd import Ensemble, Problem
    f = tmp_path / 'base.yaml'
    f.write_text(yaml.safe_dump(BASE))
    monkeypatch.setattr(Problem, 'from_string', classmethod(lambda cls, *a, **k: pytest.fail("a Problem was built")))
    with pytest.raises(KeyError):
        Ensemble.sweep(f, {'geometry.nope': [1.]})          # read, parsed and refused: no TypeError for a pathlib.Path
    with pytest.raises(KeyError):
        Ensemble.sweep(str(f), {'geometry.nope': [1.]})
