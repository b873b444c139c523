"""Elastic deformation of the gap on x-slabs (gpf_elastic_slab_*, gapflow_amd/slab.py: SlabElastic) on one GPU: the ranks
are threads of this process (gapflow_amd.slab.ThreadWorld), each a real SlabProblem with its own handle, partition, ky
column slab and seam block; the two all-to-alls and the reference all-gather are device copies.  Checked against the
undivided Problem on the same GPU and against oracle/elastic.py at the tolerances of tests/test_gpu_elastic.py.  The
distributed transform splits the FFT differently from the undivided 2-D one, so agreement is to rounding, not bitwise.
Reference: none (the reference is single-process)."""
import ctypes as C
import io
import warnings

import numpy as np
import pytest

from test_gpu_elastic import BASE, CASES, DN

pytestmark = pytest.mark.gpu

NSTEPS = 25
SLAB_CASES = {name: dict(c, grid=c['grid'].replace('Nx: 48', 'Nx: 47')) for name, c in CASES.items()}   # 47 rows: ragged cuts
# the periodic seam on the elastic path: x periodic, y free
SLAB_CASES['x_periodic_2d'] = dict(grid=f"Lx: 0.0762, Ly: 0.04, Nx: 47, Ny: 30, yS: ['D', 'N', 'N'], yN: ['D', 'N', 'N'], "
                                        "yS_D: 850., yN_D: 850.", V=0.3, alpha=0.05, images='')
RUNS = [(name, w) for name in sorted(SLAB_CASES) for w in (2, 3, 4)] + [('example_1d', 5)]

_serial = {}


def _text(name):
    return BASE.format(**SLAB_CASES[name])


def _reference(name):
    """The undivided Problem and the oracle after NSTEPS steps (computed once per case)."""
    if name not in _serial:
        from gapflow_amd import Problem
        from oracle.problem import OracleProblem
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            gpu, cpu = Problem.from_string(_text(name)), OracleProblem.from_string(_text(name))
        gpu._pre_run()
        cpu._pre_run()
        for _ in range(NSTEPS):
            gpu.update()
            cpu.update()
        assert gpu.step == cpu.step == NSTEPS
        _serial[name] = dict(step=gpu.step, dt=gpu.dt, q=gpu.q.copy(), topo=gpu.topo.full.copy(),
                             oq=cpu.q.copy(), otopo=np.concatenate([cpu.topo[:3], cpu.deformation[None]]))
        del gpu
    return _serial[name]


def _run_slabs(name, world, nsteps=NSTEPS):
    import torch
    from gapflow_amd import _lib
    from gapflow_amd.slab import SlabProblem, ThreadWorld

    def rank_body(group):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            slab = SlabProblem.from_string(_text(name), device=0, dist=group)
        slab.pre_run()
        slab.advance(nsteps)
        st = slab.state()
        topo = np.concatenate([slab._download(_lib.FIELD_TOPO, 3), slab._download(_lib.FIELD_DEFORMATION, 1)])
        return slab.layout, slab._elastic.plan, st, slab.local_q(), topo

    return ThreadWorld(world, torch).run(rank_body)


def _close(a, b, tol, what):
    scale = np.abs(b).max() or 1.0
    err = np.abs(a - b).max() / scale
    assert err <= tol, f'{what}: max difference {err:.3e} of the field scale'
    return err


@pytest.mark.parametrize('name,world', RUNS, ids=[f'{n}-{w}ranks' for n, w in RUNS])
def test_elastic_slabs_match_the_undivided_run(hiplib, name, world):
    ref = _reference(name)
    runs = _run_slabs(name, world)
    dts = [st.dt for _, _, st, _, _ in runs]
    assert len(set(dts)) == 1, f'dt differs between ranks: {dts}'
    np.testing.assert_allclose(dts[0], ref['dt'], rtol=1e-10)
    if name == 'example_1d' and world == 5:
        assert any(P.ky[r][1] == 0 for r, (_, P, _, _, _) in enumerate(runs)), 'one rank should hold no ky column'
    worst = {}
    for L, P, st, q, topo in runs:
        assert int(st.step) == ref['step'] and int(st.invalid) == 0
        rows = slice(L.lo - 1, L.hi + 2)            # owned rows and the two outer rows
        for c in range(3):
            worst['q'] = max(worst.get('q', 0), _close(q[c], ref['q'][c, rows], 1e-10, f'rank {L.rank} q[{c}]'))
        np.testing.assert_allclose(topo[0], ref['topo'][0, rows], rtol=1e-12)
        for k, what in ((1, 'dh/dx'), (2, 'dh/dy'), (3, 'deformation')):
            scale = np.abs(ref['topo'][k]).max() or 1.0
            err = np.abs(topo[k] - ref['topo'][k, rows]).max() / scale
            assert err <= 1e-9, f'rank {L.rank} {what}: {err:.3e}'
            worst[what] = max(worst.get(what, 0), err)
        # against the oracle at the tolerances of tests/test_gpu_elastic.py
        for c in range(3):
            scale = np.abs(ref['oq'][c]).max() or 1.
            assert np.abs(q[c] - ref['oq'][c, rows]).max() <= 1e-9 * scale
        od = ref['otopo'][3]
        np.testing.assert_allclose(topo[3], od[rows], rtol=1e-9, atol=1e-12 * np.abs(od).max())
        np.testing.assert_allclose(topo[0], ref['otopo'][0, rows], rtol=1e-12)
        for k in (1, 2):
            np.testing.assert_allclose(topo[k], ref['otopo'][k, rows], rtol=1e-9, atol=1e-9 * np.abs(ref['otopo'][k]).max())
    assert max(np.abs(t[3]).max() for _, _, _, _, t in runs) > 0
    print(f'{name} on {world} slabs, max difference / scale vs the undivided run: ' +
          ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))


def test_elastic_slabs_run_writes_the_serial_frames(hiplib, tmp_path):
    """The shortened 1-D example (tests/test_gpu_elastic.py) through SlabProblem.run() on 3 ranks: sol.nc and topo.nc
    with as many frames as the serial run, the deformed topography frames within 1e-9 of the serial run's."""
    import torch
    from scipy.io import netcdf_file
    from gapflow_amd import Problem
    from gapflow_amd.slab import SlabProblem, ThreadWorld
    base = BASE.format(**CASES['example_1d'])

    def text(d):
        return base.replace("options: {silent: True}", f"options: {{output: {tmp_path / d}, write_freq: 20, use_tstamp: False}}")

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        serial = Problem.from_string(text('serial'))
    serial.run()

    def rank_body(group):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            slab = SlabProblem.from_string(text('slabs'), device=0, dist=group)
        return int(slab.run().step)

    steps = ThreadWorld(3, torch).run(rank_body)
    assert steps == [serial.step] * 3

    def frames(d):
        with netcdf_file(str(tmp_path / d / 'topo.nc'), mmap=False) as f, netcdf_file(str(tmp_path / d / 'sol.nc'), mmap=False) as g:
            return f.variables['topography'][:].copy(), g.variables['solution'][:].shape[0]

    (t_ser, n_ser), (t_slab, n_slab) = frames('serial'), frames('slabs')
    assert n_slab == n_ser and t_slab.shape == t_ser.shape
    assert np.abs(t_slab[-1, 3]).max() > 0
    for c in range(4):
        scale = np.abs(t_ser[:, c]).max() or 1.0
        assert np.abs(t_slab[:, c] - t_ser[:, c]).max() <= 1e-9 * scale, c


def test_destroy_waits_for_queued_elastic_work(hiplib):
    """Slab handles destroyed straight after an elastic step was enqueued (no synchronisation in between): gpf_destroy
    drains the handle's stream before it frees the transform buffers, and a new handle's state round-trips."""
    import torch
    from gapflow_amd import Problem, _lib
    from gapflow_amd.slab import SlabProblem, ThreadWorld
    text = _text('free_2d')

    def rank_body(group):
        slab = SlabProblem.from_string(text, device=0, dist=group)
        slab.pre_run()
        slab._stagewise_step(1000, 0)          # the elastic phases are only enqueued when this returns
        group.barrier()
        _lib.check(slab.lib.gpf_destroy(slab._h))
        slab._h.value = None
        return True

    assert ThreadWorld(3, torch).run(rank_body) == [True] * 3
    p = Problem.from_string(text)
    q = np.random.default_rng(1).uniform(800., 900., (3,) + p._shape)
    p._upload(_lib.FIELD_Q, q)
    assert np.array_equal(p._download(_lib.FIELD_Q, 3), q)
    torch.cuda.synchronize()
