"""Resampling a state onto another grid, the parts that need no GPU: the index and weight rule
(gapflow_amd.resample.axis_weights), the per-cell arithmetic of csrc/resample.hpp built for the host under the sanitizers and held
against the NumPy restatement (tests/resample_cases.py), the refusals that are decided before any library call, and the
`options.init_from` key of the YAML text."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import reference_suite as rs
import resample_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostcheck', 'resample_host.cpp')


# ---- axis_weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_src, n_dst', [(50, 100), (100, 50), (12, 30), (30, 12), (10, 25), (64, 64), (1, 7), (7, 1)])
def test_axis_weights_indices_weights_and_linear_functions(n_src, n_dst):
    """Indices within 0..n_src, weights in [0, 1), and a linear function of x sampled at the source's ghosted cell centres
    comes back at the destination's centres to 1e-15 of its largest magnitude (the rule is exact for linear functions up to
    the rounding of s, of the weights' products and of one sum)."""
    from gapflow_amd.resample import axis_weights
    length = 1.0e-3
    d_src, d_dst = length / n_src, length / n_dst
    i0, w = axis_weights(n_dst, d_dst, d_src)
    assert i0.shape == w.shape == (n_dst,)
    assert i0.min() >= 0 and i0.max() <= n_src
    assert w.min() >= 0.0 and w.max() < 1.0
    i0b, wb = axis_weights(n_dst, d_dst, d_src, n_src)
    assert np.array_equal(i0, i0b) and np.array_equal(w, wb)
    x_src = (np.arange(n_src + 2) - 0.5) * d_src
    x_dst = (np.arange(1, n_dst + 1) - 0.5) * d_dst
    for a, b in ((3.0, 2.0e3), (-1.0, 7.0e2), (0.25, -4.0e3)):
        f = a + b * x_src
        got = (1.0 - w) * f[i0] + w * f[i0 + 1]
        want = a + b * x_dst
        assert np.abs(got - want).max() <= 1e-15 * np.abs(f).max(), (n_src, n_dst, a, b, np.abs(got - want).max() / np.abs(f).max())


def test_axis_weights_identity_and_extent_one():
    from gapflow_amd.resample import axis_weights
    i0, w = axis_weights(16, 2.5e-5, 2.5e-5)
    assert i0.tolist() == list(range(1, 17)) and not w.any()
    i0, w = axis_weights(1, 1.0, 1.0)
    assert i0.tolist() == [1] and w.tolist() == [0.0]
    # 50 -> 100: every fine centre sits a quarter of a coarse cell beside a coarse centre
    i0, w = axis_weights(100, 1e-5, 2e-5)
    assert i0.tolist() == [(i + 1) // 2 for i in range(100)]
    assert np.array_equal(w, np.where(np.arange(100) % 2 == 0, 0.75, 0.25))
    with pytest.raises(ValueError):
        axis_weights(0, 1.0, 1.0)
    with pytest.raises(ValueError):
        axis_weights(4, 1.0, 0.0)


# ---- resample_cell, built for the host under the sanitizers ----------------------------------------------------------------
@pytest.fixture(scope='module')
def resample_host(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is part of the image'
    exe = str(tmp_path_factory.mktemp('hostcheck') / 'resample_host')
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror', SRC, '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def smooth_fields(rng, nx, ny):
    """rho, jx, jy, h on the ghosted grid: smooth, all three fields varying, rho and h positive."""
    x = (np.arange(nx + 2) - 0.5)[:, None] / nx
    y = (np.arange(ny + 2) - 0.5)[None, :] / ny
    ph = rng.uniform(0, 2 * np.pi, 8)
    rho = 877.7 * (1.0 + 0.01 * np.sin(2 * np.pi * x + ph[0]) * np.cos(2 * np.pi * y + ph[1]))
    jx = 40.0 * (1.0 + 0.3 * np.cos(2 * np.pi * x + ph[2]) + 0.1 * np.sin(2 * np.pi * y + ph[3]))
    jy = 5.0 * np.sin(2 * np.pi * x + ph[4]) * np.sin(2 * np.pi * y + ph[5])
    h = 1.0e-5 * (1.0 + 0.7 * np.cos(2 * np.pi * x + ph[6]) * (1.0 + 0.1 * np.cos(2 * np.pi * y + ph[7])))
    return np.stack([rho, jx, jy]), h


@pytest.mark.parametrize('case', sorted(rc.GRID_PAIRS))
def test_resample_cell_matches_numpy_under_sanitizers(resample_host, case):
    """csrc/resample.hpp over whole grids (tests/hostcheck/resample_host.cpp) against the NumPy restatement: within 1e-13 of each
    field's largest magnitude, without a word from the sanitizers."""
    (nxs, nys), (nxd, nyd) = rc.GRID_PAIRS[case]
    rng = np.random.default_rng(11)
    lx, ly = 1.0e-3, 4.0e-4
    d_src, d_dst = (lx / nxs, ly / nys), (lx / nxd, ly / nyd)
    q, h = smooth_fields(rng, nxs, nys)
    _, h_dst = smooth_fields(rng, nxd, nyd)
    data = np.concatenate([[nxs, nys, nxd, nyd, d_src[0], d_src[1], d_dst[0], d_dst[1]], q.ravel(), h.ravel(), h_dst.ravel()]).astype(np.float64)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([resample_host], input=data.tobytes(), capture_output=True, env=env)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    assert res.stderr == b'', 'sanitizer output:\n' + res.stderr.decode()[-3000:]
    got = np.frombuffer(res.stdout, dtype=float).reshape(3, nxd, nyd)
    want = rc.numpy_resample(q, h, h_dst, d_src, d_dst)
    for c, name in enumerate(('rho', 'jx', 'jy')):
        err = np.abs(got[c] - want[c]).max() / np.abs(want[c]).max()
        assert err <= 1e-13, f'case {case}, {name}: {err:.2e}'
    if case == 'f':         # identity: weight 0 everywhere, rho is the source's bit for bit
        assert np.array_equal(got[0].view(np.uint64), q[0, 1:-1, 1:-1].view(np.uint64))


def test_resample_host_extent_one_copies_the_single_line(resample_host):
    """Ny = 1 on both sides: weight 0 along y, whatever the y spacing; the y ghost cells are never blended in."""
    rng = np.random.default_rng(5)
    q, h = smooth_fields(rng, 50, 1)
    q[:, :, 0] = 1e30
    q[:, :, 2] = -1e30
    _, h_dst = smooth_fields(rng, 100, 1)
    data = np.concatenate([[50, 1, 100, 1, 2e-5, 1.0, 1e-5, 1.0], q.ravel(), h.ravel(), h_dst.ravel()]).astype(np.float64)
    res = subprocess.run([resample_host], input=data.tobytes(), capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert res.returncode == 0 and res.stderr == b'', res.stderr.decode()[-3000:]
    got = np.frombuffer(res.stdout, dtype=float).reshape(3, 100, 1)
    want = rc.numpy_resample(q, h, h_dst, (2e-5, 1.0), (1e-5, 1.0))
    assert np.isfinite(got).all()
    for c in range(3):
        assert np.abs(got[c] - want[c]).max() <= 1e-13 * np.abs(want[c]).max()


# ---- refusals before the device -------------------------------------------------------------------------------------------
def grid_of(text):
    from gapflow_amd.io import read_yaml_input
    with io.StringIO(text) as f:
        return read_yaml_input(f)['grid']


def test_slab_problem_refuses_init_from():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='SlabProblem'):
        SlabProblem.init_from(object(), 'coarse/checkpoint.gpf')
    with pytest.raises(NotImplementedError, match='init_from'):
        SlabProblem({'options': {'init_from': 'coarse/checkpoint.gpf'}})


def test_geometry_mismatches_raise_value_error_from_dictionaries_alone():
    from gapflow_amd.resample import check_geometry, check_axes
    fine = grid_of(rs.JOURNAL_1D)
    coarse = grid_of(rs.JOURNAL_1D.replace('Nx: 100', 'Nx: 50').replace('dx: 1.e-5', 'dx: 2.e-5'))
    check_geometry(fine, coarse)
    check_geometry(coarse, fine)
    (i0, w), (j0, v) = check_axes(fine, coarse)
    assert i0.max() == 50 and j0.tolist() == [1] and v.tolist() == [0.0]
    longer = grid_of(rs.JOURNAL_1D.replace('Nx: 100', 'Nx: 50').replace('dx: 1.e-5', 'dx: 2.00001e-5'))
    with pytest.raises(ValueError, match='Lx'):
        check_geometry(fine, longer)
    wider = grid_of(rs.JOURNAL_1D.replace('Nx: 100', 'Nx: 50').replace('dx: 1.e-5', 'dx: 2.e-5').replace('dy: 1.', 'dy: 2.'))
    with pytest.raises(ValueError, match='Ly'):
        check_geometry(fine, wider)
    within = grid_of(rs.JOURNAL_1D.replace('Nx: 100', 'Nx: 50').replace('dx: 1.e-5', f'dx: {2.e-5 * (1 + 1e-13)!r}'))
    check_geometry(fine, within)
    walls = grid_of(rs.JOURNAL_1D.replace('Nx: 100', 'Nx: 50').replace('dx: 1.e-5', 'dx: 2.e-5')
                    .replace("xE: ['P', 'P', 'P']", "xE: ['D', 'N', 'N']").replace("xW: ['P', 'P', 'P']", "xW: ['D', 'N', 'N']"))
    with pytest.raises(ValueError, match='periodic'):
        check_geometry(fine, walls)
    with pytest.raises(ValueError, match='periodic'):
        check_geometry(walls, fine)


# ---- options.init_from of the YAML text -------------------------------------------------------------------------------------
@pytest.fixture
def dictionaries(monkeypatch):
    """Problem.from_string / from_yaml up to the dictionaries they would build the problem from (no device)."""
    from gapflow_amd import problem
    monkeypatch.setattr(problem.Problem, '_from_dict', classmethod(lambda cls, d, device=0: d))
    return problem.Problem


def test_yaml_init_from_reaches_the_options(dictionaries, tmp_path, capsys):
    text = rs.JOURNAL_1D.replace('silent: True', 'silent: True\n    init_from: coarse/checkpoint.gpf')
    d = dictionaries.from_string(text)
    assert d['options']['init_from'] == os.path.normpath(os.path.join(os.getcwd(), 'coarse/checkpoint.gpf'))
    sub = tmp_path / 'inputs'
    sub.mkdir()
    (sub / 'fine.yaml').write_text(text)
    d = dictionaries.from_yaml(str(sub / 'fine.yaml'))
    assert d['options']['init_from'] == str(sub / 'coarse' / 'checkpoint.gpf'), 'a relative path is relative to the YAML file'
    (sub / 'abs.yaml').write_text(text.replace('coarse/checkpoint.gpf', '/data/ck.gpf'))
    assert dictionaries.from_yaml(str(sub / 'abs.yaml'))['options']['init_from'] == '/data/ck.gpf'
    # the command line's path replaces the file's and is relative to the working directory
    d = dictionaries.from_yaml(str(sub / 'fine.yaml'), init_from='other.gpf')
    assert d['options']['init_from'] == os.path.abspath('other.gpf')
    with pytest.raises(ValueError, match='init_from'):
        dictionaries.from_string(text.replace('coarse/checkpoint.gpf', '[1, 2]'))
    capsys.readouterr()


def test_yaml_without_init_from_is_unchanged(dictionaries):
    """Absent: no key appears, and the dictionaries are those of the stages before this key existed."""
    from gapflow_amd import problem
    from gapflow_amd.io import read_yaml_input
    d = dictionaries.from_string(rs.JOURNAL_1D)
    assert 'init_from' not in d['options']
    with io.StringIO(rs.JOURNAL_1D) as f:
        want = read_yaml_input(f)
    problem._keep_checkpoint_freq(want, rs.JOURNAL_1D)
    problem._keep_probes(want, rs.JOURNAL_1D)
    problem._keep_integrals(want, rs.JOURNAL_1D)
    problem._keep_extrema(want, rs.JOURNAL_1D)
    assert d == want


def test_command_line_takes_init_from():
    from gapflow_amd.__main__ import make_parser
    opts = make_parser().parse_args(['-i', 'fine.yaml', '--init-from', 'coarse_out/checkpoint.gpf'])
    assert opts.filename == 'fine.yaml' and opts.init_from == 'coarse_out/checkpoint.gpf'
    assert make_parser().parse_args(['-i', 'fine.yaml']).init_from is None
