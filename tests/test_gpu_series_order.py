"""The summation order of the row-reduced series (csrc/series_rows.hpp: row_pairs, block_sum, fold_rows), pinned without a second
library to compare with: the weighted integrals' `h` column is the sum of w * h with every product rounded on its own
(csrc/weighted_kernels.hip: wfilm_cell), so NumPy reproduces each term exactly and the documented tree can be replayed on the host:
    per interior row, thread t of 256 adds its column pairs (1 + 2k, 2 + 2k), k = t, t + 256, ..., lower column first, to +0.0;
    the lanes of each of the four waves fold 32, 16, .. 1 apart; the four wave sums are added in order to +0.0;
    fold thread t adds the row sums t, t + 256, ... in order to +0.0; the same tree folds the 256 threads;
    the result times dx * dy.
film_weighted() and film_regions() of an uploaded state (no step is taken) are held to the replay bit for bit, with the 16-byte
and the 8-byte pair loads.  Shapes (Nx, Ny): (3, 1) a lone half pair; (5, 2); (2, 129) 65 pairs, a second wave with one lane;
(6, 601) a second pair per thread and an odd end; (300, 7) a second row per fold thread.  Weights in [0.5, 1.5) and gap heights in
[1e-6, 1e-5) from a fixed seed; on every shape but the two smallest, math.fsum of the same terms differs from the replay, so
another order would show.  Reference: none (post-processing there)."""
import math

import numpy as np
import pytest

import test_gpu_probes as tp
from test_gpu_probes import DN, bits

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1), (5, 2), (2, 129), (6, 601), (300, 7)]
DISCRIMINATES = SHAPES[2:]
SEED = 20261059                         # checked: every shape of DISCRIMINATES differs from fsum
H_LO, H_HI = 3.0e-6, 7.0e-6             # the region: h in [H_LO, H_HI)

TEXT = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, dx: 1.3e-4, dy: 1.7e-4, {bc}, xE_D: 877.7007, xW_D: 877.7007}}
geometry: {{type: inclined, hmax: 1.2e-5, hmin: 4.e-6, U: 0.5, V: 0.}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: 0, tol: 1e-14, dt: 2.e-9, max_it: 100000}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}}
"""


def inputs(nx, ny):
    """(w, h), each (nx, ny) over the interior cells"""
    rng = np.random.default_rng([SEED, nx, ny])
    return 0.5 + rng.random((nx, ny)), 1.0e-6 + 9.0e-6 * rng.random((nx, ny))


def block_sum(threads):
    """The value thread 0 holds after block_sum: `threads` are the 256 threads' sums"""
    v = np.array(threads, dtype=np.float64).reshape(4, 64)
    for s in (32, 16, 8, 4, 2, 1):
        v[:, :64 - s] = v[:, :64 - s] + v[:, s:]            # (lanes whose partner lies beyond the wave never reach lane 0)
    r = np.float64(0.0)
    for wave in range(4):
        r = r + v[wave, 0]
    return r


def replay(terms, dA):
    """The record's value for the cells' terms (nx, ny), each already rounded"""
    nx, ny = terms.shape
    rows = []
    for ix in range(nx):
        threads = [np.float64(0.0)] * 256
        for k in range((ny + 1) // 2):
            a = threads[k % 256] + terms[ix, 2 * k]
            if 2 * k + 1 < ny:
                a = a + terms[ix, 2 * k + 1]
            threads[k % 256] = a
        rows.append(block_sum(threads))
    threads = [np.float64(0.0)] * 256
    for row in range(nx):
        threads[row % 256] = threads[row % 256] + rows[row]
    return block_sum(threads) * dA


def same_bits(a, b):
    return int(bits(a).ravel()[0]) == int(bits(b).ravel()[0])


@pytest.mark.parametrize('narrow', [False, True], ids=['wide', 'narrow'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h_sums_follow_the_documented_tree(hiplib, monkeypatch, shape, narrow):
    nx, ny = shape
    if narrow:
        monkeypatch.setenv('GPF_FILM_NARROW', '1')          # read by gpf_weighted_set and gpf_regions_set
    else:
        monkeypatch.delenv('GPF_FILM_NARROW', raising=False)
    w, h = inputs(nx, ny)
    p = tp.build(TEXT.format(nx=nx, ny=ny, bc=DN))
    gap = np.array(p.topo.full[0])
    gap[1:-1, 1:-1] = h
    p.topo.full[0] = gap
    p._upload_topo()
    dA = p.grid['dx'] * p.grid['dy']

    p.set_weighted_integrals(w)
    got = p.film_weighted()['h'][0]
    want = replay(w * h, dA)
    exact = math.fsum((w * h).ravel()) * dA
    print(f"\n[{nx} x {ny}, {'8' if narrow else '16'}-byte loads] weighted h {got!r}, replay {want!r}, fsum {exact!r}")
    assert same_bits(got, want), f"weighted h {got!r} against the replay {want!r}"
    if shape in DISCRIMINATES:
        assert not same_bits(want, exact), "the inputs do not tell this order from an exact sum"

    member = (h >= H_LO) & (h < H_HI)
    p.set_regions([{'field': 'h', 'above': H_LO, 'below': H_HI}])
    rec = p.film_regions()
    want = replay(np.where(member, 1.0, 0.0) * h, dA)
    print(f"region h {rec['h'][0]!r}, replay {want!r}, cells {int(rec['cells'][0])}, bbox {rec['bbox'][0].tolist()}")
    assert same_bits(rec['h'][0], want), f"region h {rec['h'][0]!r} against the replay with 0 / 1 weights {want!r}"
    ix, iy = np.nonzero(member)
    assert int(rec['cells'][0]) == ix.size
    assert rec['bbox'][0].tolist() == ([ix.min() + 1, ix.max() + 1, iy.min() + 1, iy.max() + 1] if ix.size else [-1, -1, -1, -1])
