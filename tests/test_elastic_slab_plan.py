"""The x-slab form of the elastic half-space convolution on the CPU: gapflow_amd/elastic.py's SlabElasticPlan (who owns,
sends and receives which transform rows and ky columns) and, over gloo, a NumPy engine that follows the device pipeline
of csrc/api_slab_elastic.inc step by step (row y-transforms, column pack, all-to-all, x-transforms and Green's multiply on
a ky slab, row pack, all-to-all, unpack, inverse y-transforms).  The rows each rank keeps must match the undivided
irfft2(rfft2(forces) * G) of oracle/elastic.py.  Reference: none (the reference is single-process)."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gapflow_amd.elastic import SlabElasticPlan, ky_partition      # noqa: E402
from gapflow_amd.slab import partition                               # noqa: E402

MODES = {'full': (True, True), 'x_periodic': (True, False), 'y_periodic': (False, True), 'none': (False, False)}


def _plan(Nx, Ny, world, mode):
    perX, perY = MODES[mode]
    nx, ny = Nx + 2, Ny + 2
    px, py = (nx if perX else 2 * nx), (ny if perY else 2 * ny)
    return SlabElasticPlan(Nx, px, py, partition(Nx, world), perX)


def _cases():
    for Nx in (1, 2, 37, 48):
        for world in range(1, 6):
            if world > Nx:
                continue
            for mode in MODES:
                yield Nx, world, mode


@pytest.mark.parametrize('Nx,world,mode', list(_cases()))
def test_plan_invariants(Nx, world, mode):
    Ny = 5
    P = _plan(Nx, Ny, world, mode)
    # transform rows: 0..Nx+1 exactly once, contiguous and in rank order
    rows = [g for r0, n in P.fwd for g in range(r0, r0 + n)]
    assert rows == list(range(Nx + 2))
    # ky columns: 0..py/2 exactly once (empty slabs allowed)
    cols = [k for k0, n in P.ky for k in range(k0, k0 + n)]
    assert cols == list(range(P.py // 2 + 1))
    assert all(n >= 0 for _, n in P.ky)
    # what r sends to s is what s expects from r, in both transposes
    for r in range(world):
        for s in range(world):
            assert P.send1(r)[s] == P.recv1(s)[r]
            assert P.send2(r)[s] == P.recv2(s)[r]
    # return rows: lo-2 .. hi+2 clipped, plus the seam rows
    perX = MODES[mode][0]
    for r, (lo, hi) in enumerate(P.parts):
        want = list(range(max(0, lo - 2), min(Nx + 1, hi + 2) + 1))
        if perX and world > 1 and r == 0:
            want += [Nx - 1, Nx, Nx + 1]
        elif perX and world > 1 and r == world - 1:
            want += [0, 1, 2]
        assert P.return_rows(r) == want
        c = P.c_plan(r)
        assert c.dtype == np.int32 and c.size == 13 + sum(len(P.return_rows(s)) for s in range(world))


def test_ky_partition_allows_empty_slabs():
    # the 1-D example (Ny = 1, y free): py = 6, four columns over five ranks
    assert ky_partition(4, 5) == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 0)]
    assert ky_partition(10, 3) == [(0, 4), (4, 3), (7, 3)]


# ---------------------------------------------------------------------------------------------
# the distributed convolution over gloo
# ---------------------------------------------------------------------------------------------

def _grid(Nx, Ny, mode):
    perX, perY = MODES[mode]
    P, F = ['P', 'P', 'P'], ['D', 'N', 'N']
    return {'Nx': Nx, 'Ny': Ny, 'Lx': 0.07, 'Ly': 0.04, 'dx': 0.07 / Nx, 'dy': 0.04 / Ny,
            'bc_xE_P': [perX] * 3, 'bc_xW_P': [perX] * 3, 'bc_yS_P': [perY] * 3, 'bc_yN_P': [perY] * 3}


def _forces(Nx, Ny):
    rng = np.random.default_rng(Nx * 100 + Ny)
    return rng.uniform(0.5, 2.0, (Nx + 2, Ny + 2)) * 1e6


def _distributed(rank, world, Nx, Ny, mode, dist, torch):
    """What each rank computes, phase by phase as on the device; returns (return rows, u on them)."""
    from oracle.elastic import ElasticDeformation
    g = _grid(Nx, Ny, mode)
    el = ElasticDeformation(210e9, 0.3, 1.0, g, 2)
    px, py = el.pad if el.periodicity != 'full' else el.n
    P = SlabElasticPlan(Nx, px, py, partition(Nx, world), MODES[mode][0])
    nky = py // 2 + 1
    f = _forces(Nx, Ny)
    # 1. forward y-transform of the owned rows, zero-padded lines of length py
    r0, nr = P.fwd[rank]
    dense = np.zeros((nr, py))
    dense[:, :Ny + 2] = f[r0:r0 + nr]
    spec = np.fft.rfft(dense, axis=1)
    # 2. column pack: chunk s = [row][k - k0(s)], then the all-to-all
    send = np.concatenate([spec[:, k0:k0 + n].reshape(-1) for k0, n in P.ky])
    recv = torch.zeros(sum(P.recv1(rank)), dtype=torch.complex128)
    dist.all_to_all_single(recv, torch.from_numpy(send), P.recv1(rank), P.send1(rank))
    k0, nk = P.ky[rank]
    cols = np.zeros((px, nk), complex)
    cols[:Nx + 2] = recv.numpy().reshape(Nx + 2, nk)      # rank order is x order: [row][local ky], zero rows complete it
    # 3. x-transform, multiply by this rank's slice of G, inverse x-transform
    cols = np.fft.ifft(np.fft.fft(cols, axis=0) * el.greens[:, k0:k0 + nk], axis=0)
    # 4. row pack of every rank's return rows, all-to-all, unpack into [row][ky] lines, inverse y-transform
    send2 = np.concatenate([cols[P.return_rows(s)].reshape(-1) for s in range(world)])
    rows = P.return_rows(rank)
    recv2 = torch.zeros(sum(P.recv2(rank)), dtype=torch.complex128)
    dist.all_to_all_single(recv2, torch.from_numpy(send2), P.recv2(rank), P.send2(rank))
    line = np.zeros((len(rows), nky), complex)
    o = 0
    for s, (ks, ns) in enumerate(P.ky):
        line[:, ks:ks + ns] = recv2.numpy()[o:o + len(rows) * ns].reshape(len(rows), ns)
        o += len(rows) * ns
    u = np.fft.irfft(line, n=py, axis=1)[:, :Ny + 2]
    ref = np.fft.irfft2(el.greens * np.fft.rfft2(np.pad(f, ((0, px - Nx - 2), (0, py - Ny - 2)))), s=(px, py))
    return rows, u, ref[rows, :Ny + 2]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        worst = {}
        for mode in MODES:
            for Nx, Ny in ((37, 11), (6, 1), (5, 4)):
                rows, u, ref = _distributed(rank, world, Nx, Ny, mode, dist, torch)
                worst[f'{mode}_{Nx}_{Ny}'] = np.abs(u - ref).max() / np.abs(ref).max()
        np.save(os.path.join(out_dir, f'rank{rank}.npy'), worst)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_distributed_convolution_over_gloo_matches_rfft2(tmp_path, world):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        worst = np.load(tmp_path / f'rank{r}.npy', allow_pickle=True).item()
        assert len(worst) == 12
        for case, err in worst.items():
            assert err < 1e-13, f'rank {r}, {case}: relative error {err:.3e}'
